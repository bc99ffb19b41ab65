// Stand-alone driver of the host side of the genotype matrix product for the sanitizer build
// of tests/test_geno_matmul_host.py (built and run by tests/host_driver.py, csrc/king_host.cc
// linked in).  Every buffer is an exact-size heap allocation, so a byte read or written past
// an end is caught.
//   1. cuking_geno_matmul_host against the sum over plain code arrays, both table axes, integer
//      operands (exact), pitches equal to and above num_rhs, pad elements untouched, garbage
//      bits beyond num_cols;
//   2. geno_code of csrc/king_geno.h on random words; the refusals; the calls without work.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <vector>

#include "cuking_amd.h"
#include "host_driver_common.h"
#include "king_geno.h"

namespace {

// (fail: what, rows, columns, right-hand sides)

void run_shape(uint32_t rows, uint32_t cols, uint32_t rhs, int axis, uint32_t ldb, uint32_t ldo) {
  const uint32_t plane = (cols + 63) / 64 + (cols % 3 == 0 ? 1 : 0);  // (room beyond num_cols too)
  const uint32_t words = 2 * (plane ? plane : 1), w = words / 2;
  std::vector<uint8_t> code((size_t)rows * cols);
  std::unique_ptr<uint64_t[]> bits(new uint64_t[(size_t)rows * words]);
  for (size_t k = 0; k < (size_t)rows * words; ++k) bits[k] = next_random();  // garbage beyond
  for (uint32_t r = 0; r < rows; ++r)
    for (uint32_t k = 0; k < cols; ++k) {
      const uint8_t c = (uint8_t)(next_random() & 3);
      code[(size_t)r * cols + k] = c;
      uint64_t &het = bits[(size_t)r * words + k / 64], &hom = bits[(size_t)r * words + w + k / 64];
      het = (het & ~(1ull << (k % 64))) | ((uint64_t)(c & 1) << (k % 64));
      hom = (hom & ~(1ull << (k % 64))) | ((uint64_t)(c >> 1) << (k % 64));
    }
  const uint32_t entries = axis == CUKING_GENO_TABLE_PER_ROW ? rows : cols;
  std::unique_ptr<float[]> table(new float[(size_t)entries * 4]);
  for (size_t k = 0; k < (size_t)entries * 4; ++k) table[k] = (float)((int)(next_random() % 7) - 3);
  // B: exactly (cols - 1) * ldb + rhs floats -- the last row has no pad
  const size_t b_size = cols ? (size_t)(cols - 1) * ldb + rhs : 0;
  std::unique_ptr<float[]> b(new float[b_size]);
  for (size_t k = 0; k < b_size; ++k) b[k] = (float)((int)(next_random() % 17) - 8);
  const size_t out_size = (size_t)(rows - 1) * ldo + rhs;
  std::unique_ptr<float[]> out(new float[out_size]);
  for (size_t k = 0; k < out_size; ++k) out[k] = -12345.0f;
  if (cuking_geno_matmul_host(bits.get(), rows, words, cols, table.get(), axis, b.get(), ldb, rhs,
                              out.get(), ldo) != CUKING_OK)
    return fail("refused", rows, cols, rhs);
  for (uint32_t r = 0; r < rows; ++r) {
    for (uint32_t c = 0; c < rhs; ++c) {
      int64_t want = 0;
      for (uint32_t k = 0; k < cols; ++k) {
        const size_t t = (size_t)(axis == CUKING_GENO_TABLE_PER_ROW ? r : k) * 4 +
                         code[(size_t)r * cols + k];
        want += (int64_t)table[t] * (int64_t)b[(size_t)k * ldb + c];
      }
      if (out[(size_t)r * ldo + c] != (float)want) return fail("sum", rows, cols, rhs);
    }
    for (uint32_t c = rhs; c < ldo && r + 1 < rows; ++c)
      if (out[(size_t)r * ldo + c] != -12345.0f) return fail("pad written", rows, cols, rhs);
  }
}

void check_helpers_and_refusals() {
  for (int round = 0; round < 2000; ++round) {
    const uint64_t het = next_random(), hom = next_random();
    for (uint32_t bit = 0; bit < 64; ++bit) {
      const uint32_t want = (uint32_t)((het >> bit) & 1) + 2 * (uint32_t)((hom >> bit) & 1);
      if (cuking::geno_code(het, hom, bit) != want) return fail("geno_code", 0, bit, 0);
    }
  }
  if (!cuking::geno_axis_valid(0) || !cuking::geno_axis_valid(1) || cuking::geno_axis_valid(2) ||
      cuking::geno_axis_valid(-1) || cuking::kGenoRhsMax != CUKING_GENO_RHS_MAX ||
      cuking::kGenoTablePerColumn != CUKING_GENO_TABLE_PER_COLUMN ||
      cuking::kGenoTablePerRow != CUKING_GENO_TABLE_PER_ROW)
    fail("constants", 0, 0, 0);
  uint64_t bits[4] = {0, 0, 0, 0};
  float table[8] = {1, 2, 3, 4, 5, 6, 7, 8}, b[2] = {1, 1}, out[2] = {9, 9};
  const cuking_status bad = CUKING_ERR_INVALID_ARGUMENT;
  if (cuking_geno_matmul_host(bits, 2, 2, 2, table, 0, b, 1, 1, out, 1) != CUKING_OK ||
      out[0] != 6.0f || out[1] != 6.0f)
    fail("valid call", 2, 2, 1);
  if (cuking_geno_matmul_host(nullptr, 2, 2, 2, table, 0, b, 1, 1, out, 1) != bad ||
      cuking_geno_matmul_host(bits, 2, 2, 2, nullptr, 0, b, 1, 1, out, 1) != bad ||
      cuking_geno_matmul_host(bits, 2, 2, 2, table, 0, nullptr, 1, 1, out, 1) != bad ||
      cuking_geno_matmul_host(bits, 2, 2, 2, table, 0, b, 1, 1, nullptr, 1) != bad ||
      cuking_geno_matmul_host(bits, 2, 1, 2, table, 0, b, 1, 1, out, 1) != bad ||
      cuking_geno_matmul_host(bits, 2, 0, 0, table, 0, b, 1, 1, out, 1) != bad ||
      cuking_geno_matmul_host(bits, 2, 2, 65, table, 0, b, 1, 1, out, 1) != bad ||
      cuking_geno_matmul_host(bits, 2, 2, 2, table, 0, b, 1, 0, out, 1) != bad ||
      cuking_geno_matmul_host(bits, 2, 2, 2, table, 0, b, 65, 65, out, 65) != bad ||
      cuking_geno_matmul_host(bits, 2, 2, 2, table, 0, b, 1, 2, out, 2) != bad ||
      cuking_geno_matmul_host(bits, 2, 2, 2, table, 0, b, 2, 2, out, 1) != bad ||
      cuking_geno_matmul_host(bits, 2, 2, 2, table, 2, b, 1, 1, out, 1) != bad)
    fail("refusals", 2, 2, 1);
  out[0] = out[1] = 9;
  if (cuking_geno_matmul_host(nullptr, 0, 2, 2, nullptr, 0, nullptr, 1, 1, nullptr, 1) != CUKING_OK ||
      cuking_geno_matmul_host(nullptr, 2, 2, 0, nullptr, 1, nullptr, 1, 1, out, 1) != CUKING_OK ||
      out[0] != 0.0f || out[1] != 0.0f)
    fail("calls without work", 0, 0, 1);
}

}  // namespace

int main() {
  const uint32_t rows[] = {1, 33, 130}, cols[] = {0, 1, 63, 64, 65, 700}, rhs[] = {1, 31, 33, 64};
  for (const uint32_t r : rows)
    for (const uint32_t k : cols)
      for (const uint32_t c : rhs)
        for (int axis = 0; axis < 2; ++axis) {
          run_shape(r, k, c, axis, c, c);
          run_shape(r, k, c, axis, c + 3, c + 5);
        }
  check_helpers_and_refusals();
  printf("%d failures\n", g_failures);
  return g_failures != 0;
}
