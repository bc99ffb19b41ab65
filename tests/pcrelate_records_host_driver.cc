// Stand-alone driver of the host side of the PC-Relate records for the sanitizer build of
// tests/test_pcrelate_records_host.py (built and run by tests/host_driver.py, csrc/king_host.cc
// linked in).  Every buffer is an exact-size heap allocation, so a byte read or written past
// an end is caught.
//   1. cuking_pcrelate_records_host in the exact setting (d = 1, X = 1, beta in {0, 1, 2})
//      against cuking_pcrelate_matrix_host of the same block thresholded: the pairs in ascending
//      (i, j), the kin bytes, the count; record buffers of exactly the count, of one less
//      (RESOURCE_EXHAUSTED, the exact count, the first count - 1 records) and the counting call
//      with a null buffer;
//   2. the tile map of csrc/king_pcrelate.h: every side up to 64 in full, the ends of the largest
//      side; the refusals; the calls without work.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "cuking_amd.h"
#include "host_driver_common.h"
#include "king_pcrelate.h"

namespace {

// (fail: what, samples, sites, one more number)

void run_shape(uint32_t n, uint32_t sites, cuking_submatrix block, float min_kin) {
  const uint32_t plane = (sites + 63) / 64 + (sites % 3 == 0 ? 1 : 0);  // (room beyond num_sites)
  const uint32_t words = 2 * (plane ? plane : 1);
  std::unique_ptr<uint64_t[]> bits(new uint64_t[(size_t)n * words]);
  for (size_t k = 0; k < (size_t)n * words; ++k) bits[k] = next_random() & next_random();
  std::unique_ptr<float[]> x(new float[n]);
  for (uint32_t k = 0; k < n; ++k) x[k] = 1.0f;
  std::unique_ptr<float[]> beta(new float[sites]);
  for (uint32_t k = 0; k < sites; ++k) beta[k] = (float)(next_random() % 3);
  const uint32_t rows = block.i_end - block.i_begin, cols = block.j_end - block.j_begin;
  std::unique_ptr<float[]> kin(new float[(size_t)rows * cols]);
  if (cuking_pcrelate_matrix_host(bits.get(), n, words, sites, x.get(), 1, beta.get(), 1, 1, 0.01f,
                                  0.99f, &block, kin.get(), cols) != CUKING_OK)
    return fail("matrix refused", n, sites, 0);
  std::vector<cuking_result> want;
  const bool diag = block.i_begin == block.j_begin;
  for (uint32_t i = 0; i < rows; ++i)
    for (uint32_t j = diag ? i + 1 : 0; j < cols; ++j)
      if (sites != 0 && kin[(size_t)i * cols + j] > min_kin)
        want.push_back({block.i_begin + i, block.j_begin + j, kin[(size_t)i * cols + j], 0, 0, 0});
  const uint64_t total = want.size();
  // the counting call
  uint64_t count = 77;
  cuking_status st = cuking_pcrelate_records_host(bits.get(), n, words, sites, x.get(), 1,
                                                  beta.get(), 1, 1, 0.01f, 0.99f, &block, min_kin,
                                                  nullptr, 0, &count);
  if (count != total || st != (total ? CUKING_ERR_RESOURCE_EXHAUSTED : CUKING_OK))
    return fail("counting call", n, sites, count);
  // a buffer of exactly the count, then of one less
  for (const uint64_t room : {total, total ? total - 1 : 0}) {
    std::unique_ptr<cuking_result[]> got(new cuking_result[room]);
    count = 77;
    st = cuking_pcrelate_records_host(bits.get(), n, words, sites, x.get(), 1, beta.get(), 1, 1,
                                      0.01f, 0.99f, &block, min_kin, room ? got.get() : nullptr,
                                      room, &count);
    if (count != total || st != (room < total ? CUKING_ERR_RESOURCE_EXHAUSTED : CUKING_OK))
      return fail("count or status", n, sites, room);
    if (room != 0 && memcmp(got.get(), want.data(), room * sizeof(cuking_result)) != 0)
      return fail("records", n, sites, room);
  }
}

void check_tile_map() {
  for (uint64_t side = 1; side <= 64; ++side) {
    uint64_t index = 0;
    for (uint32_t i = 0; i < side; ++i)
      for (uint32_t j = i; j < side; ++j, ++index) {
        uint32_t ti = ~0u, tj = ~0u;
        cuking::pcrelate_triangle_tile(side, index, &ti, &tj);
        if (ti != i || tj != j || cuking::pcrelate_triangle_index(side, i, j) != index)
          return fail("tile map", (uint32_t)side, 0, index);
      }
    if (index != cuking::pcrelate_triangle_tiles(side)) return fail("tile count", (uint32_t)side, 0, index);
  }
  const uint64_t side = CUKING_PCRELATE_TRIANGLE_SIDE_MAX;
  if (side != cuking::kPcrelateTriangleSideMax || side != (0xFFFFFFFFull + 127) / 128)
    return fail("largest side", 0, 0, side);
  const uint64_t total = cuking::pcrelate_triangle_tiles(side);
  for (uint64_t index = 0; index < 1000; ++index) {
    uint32_t ti = ~0u, tj = ~0u;
    cuking::pcrelate_triangle_tile(side, index, &ti, &tj);
    if (ti != 0 || tj != index) return fail("first tiles", 0, 0, index);
  }
  // from the end: rows of 1, 2, 3, ... tiles
  uint64_t index = total;
  for (uint64_t m = 0; total - index < 1000; ++m)
    for (uint64_t k = 0; k <= m; ++k) {
      --index;
      uint32_t ti = ~0u, tj = ~0u;
      cuking::pcrelate_triangle_tile(side, index, &ti, &tj);
      if (ti != side - 1 - m || tj != side - 1 - k ||
          cuking::pcrelate_triangle_index(side, ti, tj) != index)
        return fail("last tiles", 0, 0, index);
    }
  uint32_t ti, tj;
  if (cuking_pcrelate_triangle_tile(side, total, &ti, &tj) != 0 ||
      cuking_pcrelate_triangle_tile(side + 1, 0, &ti, &tj) != 0 ||
      cuking_pcrelate_triangle_tile(side, 0, nullptr, &tj) != 0 ||
      cuking_pcrelate_triangle_tile(side, total - 1, &ti, &tj) != 1 || ti != side - 1 ||
      tj != side - 1 || cuking_pcrelate_triangle_tiles(side) != total ||
      cuking_pcrelate_triangle_tiles(side + 1) != 0 ||
      cuking_pcrelate_triangle_index(side, 3, 2) != UINT64_MAX)
    fail("exported tile map", 0, 0, 0);
}

void check_refusals() {
  uint64_t bits[4] = {0, 0, 0, 0};  // two samples, one plane word: hom-ref everywhere
  float x[2] = {1, 1}, beta[2] = {1, 1};
  cuking_result rec[1] = {{9, 9, 9.0f, 9, 9, 9}};
  uint64_t count = 77;
  cuking_submatrix whole = {0, 2, 0, 2}, outside = {0, 3, 0, 3}, reversed = {2, 1, 2, 1};
  cuking_submatrix overlap = {0, 2, 1, 2}, empty = {1, 1, 0, 2}, one = {1, 2, 1, 2};
  const cuking_status bad = CUKING_ERR_INVALID_ARGUMENT;
  // (r = -1, v = 0.5 at both sites: kin = 2 / (4 * 0.5) = 1)
  if (cuking_pcrelate_records_host(bits, 2, 2, 2, x, 1, beta, 1, 1, 0.01f, 0.99f, &whole, 0.5f, rec,
                                   1, &count) != CUKING_OK ||
      count != 1 || rec[0].sample_i != 0 || rec[0].sample_j != 1 || rec[0].kin != 1.0f ||
      rec[0].ibs0 != 0 || rec[0].ibs1 != 0 || rec[0].ibs2 != 0)
    fail("valid call", 2, 2, count);
  // (kin > 1.0f is false: the strict comparison)
  if (cuking_pcrelate_records_host(bits, 2, 2, 2, x, 1, beta, 1, 1, 0.01f, 0.99f, &whole, 1.0f, rec,
                                   1, &count) != CUKING_OK || count != 0)
    fail("strict comparison", 2, 2, count);
  rec[0] = {9, 9, 9.0f, 9, 9, 9};
#define REFUSED(...) (count = 77, cuking_pcrelate_records_host(__VA_ARGS__) != bad || count != 0)
  if (REFUSED(nullptr, 2, 2, 2, x, 1, beta, 1, 1, 0.01f, 0.99f, &whole, 0.0f, rec, 1, &count) ||
      REFUSED(bits, 2, 2, 2, nullptr, 1, beta, 1, 1, 0.01f, 0.99f, &whole, 0.0f, rec, 1, &count) ||
      REFUSED(bits, 2, 2, 2, x, 1, nullptr, 1, 1, 0.01f, 0.99f, &whole, 0.0f, rec, 1, &count) ||
      REFUSED(bits, 2, 2, 2, x, 1, beta, 1, 1, 0.01f, 0.99f, &whole, 0.0f, nullptr, 1, &count) ||
      REFUSED(bits, 2, 2, 2, x, 1, beta, 1, 1, 0.01f, 0.99f, &whole, NAN, rec, 1, &count) ||
      REFUSED(bits, 2, 2, 2, x, 1, beta, 1, 1, 0.01f, 0.99f, nullptr, 0.0f, rec, 1, &count) ||
      REFUSED(bits, 2, 1, 2, x, 1, beta, 1, 1, 0.01f, 0.99f, &whole, 0.0f, rec, 1, &count) ||
      REFUSED(bits, 2, 2, 65, x, 1, beta, 1, 1, 0.01f, 0.99f, &whole, 0.0f, rec, 1, &count) ||
      REFUSED(bits, 2, 2, 2, x, 1, beta, 1, 0, 0.01f, 0.99f, &whole, 0.0f, rec, 1, &count) ||
      REFUSED(bits, 2, 2, 2, x, 33, beta, 33, 33, 0.01f, 0.99f, &whole, 0.0f, rec, 1, &count) ||
      REFUSED(bits, 2, 2, 2, x, 1, beta, 2, 2, 0.01f, 0.99f, &whole, 0.0f, rec, 1, &count) ||
      REFUSED(bits, 2, 2, 2, x, 1, beta, 1, 1, 0.5f, 0.5f, &whole, 0.0f, rec, 1, &count) ||
      REFUSED(bits, 2, 2, 2, x, 1, beta, 1, 1, NAN, 0.99f, &whole, 0.0f, rec, 1, &count) ||
      REFUSED(bits, 2, 2, 2, x, 1, beta, 1, 1, 0.01f, 0.99f, &outside, 0.0f, rec, 1, &count) ||
      REFUSED(bits, 2, 2, 2, x, 1, beta, 1, 1, 0.01f, 0.99f, &reversed, 0.0f, rec, 1, &count) ||
      REFUSED(bits, 2, 2, 2, x, 1, beta, 1, 1, 0.01f, 0.99f, &overlap, 0.0f, rec, 1, &count))
    fail("refusals", 2, 2, 1);
#undef REFUSED
  if (cuking_pcrelate_records_host(bits, 2, 2, 2, x, 1, beta, 1, 1, 0.01f, 0.99f, &whole, 0.0f, rec,
                                   1, nullptr) != bad)
    fail("null num_records", 2, 2, 1);
  if (rec[0].sample_i != 9 || rec[0].kin != 9.0f || rec[0].ibs2 != 9)
    fail("a refused call wrote", 2, 2, 1);
  // without work: an empty block, a 1 x 1 diagonal block, no sites -- null pointers allowed
  for (const cuking_submatrix *b : {&empty, &one, &whole}) {
    count = 77;
    const uint32_t sites = b == &whole ? 0 : 2;
    const bool work = b == &one;  // (a 1 x 1 diagonal block reads its sample, and finds no pair)
    if (cuking_pcrelate_records_host(work ? bits : nullptr, 2, 2, sites, work ? x : nullptr, 1,
                                     work ? beta : nullptr, 1, 1, 0.01f, 0.99f, b,
                                     -INFINITY, nullptr, 0, &count) != CUKING_OK || count != 0)
      fail("calls without work", 0, sites, count);
  }
}

}  // namespace

int main() {
  const uint32_t samples[] = {1, 33, 130}, sites[] = {0, 1, 63, 64, 65, 700};
  for (const uint32_t n : samples)
    for (const uint32_t s : sites)
      for (const float t : {-INFINITY, 0.0f, 0.25f, INFINITY}) {
        run_shape(n, s, {0, n, 0, n}, t);
        if (n >= 33) run_shape(n, s, {5, 20, 21, n}, t);
        run_shape(n, s, {n - 1, n, n - 1, n}, t);
      }
  check_tile_map();
  check_refusals();
  printf("%d failures\n", g_failures);
  return g_failures != 0;
}
