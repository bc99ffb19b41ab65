// Stand-alone driver of the host side of PC-Relate for the sanitizer build of
// tests/test_pcrelate_host.py (built and run by tests/host_driver.py, csrc/king_host.cc linked in).
// Every buffer is an exact-size heap allocation, so a byte read or written past an end is
// caught.
//   1. cuking_pcrelate_matrix_host in the exact setting (d = 1, X = 1, beta in {0, 1, 2}: num an
//      integer, 4 den a count) against the integer formula on plain code arrays, diagonal and
//      off-diagonal blocks, pitches equal to and above the need, pad elements untouched,
//      garbage bits beyond num_sites;
//   2. the element functions of csrc/king_pcrelate.h; the refusals; the calls without work.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <vector>

#include "cuking_amd.h"
#include "host_driver_common.h"
#include "king_pcrelate.h"

namespace {

// (fail: what, samples, sites, one more number)

void run_shape(uint32_t n, uint32_t sites, cuking_submatrix block, uint32_t pad) {
  const uint32_t plane = (sites + 63) / 64 + (sites % 3 == 0 ? 1 : 0);  // (room beyond num_sites)
  const uint32_t words = 2 * (plane ? plane : 1), w = words / 2;
  std::vector<uint8_t> code((size_t)n * sites);
  std::unique_ptr<uint64_t[]> bits(new uint64_t[(size_t)n * words]);
  for (size_t k = 0; k < (size_t)n * words; ++k) bits[k] = next_random();  // garbage beyond
  for (uint32_t i = 0; i < n; ++i)
    for (uint32_t s = 0; s < sites; ++s) {
      const uint8_t c = (uint8_t)(next_random() & 3);
      code[(size_t)i * sites + s] = c;
      uint64_t &het = bits[(size_t)i * words + s / 64], &hom = bits[(size_t)i * words + w + s / 64];
      het = (het & ~(1ull << (s % 64))) | ((uint64_t)(c & 1) << (s % 64));
      hom = (hom & ~(1ull << (s % 64))) | ((uint64_t)(c >> 1) << (s % 64));
    }
  const uint32_t ldx = 1 + pad, ldbeta = 1 + pad;
  // X and beta: exactly (rows - 1) * pitch + 1 floats -- the last row has no pad
  std::unique_ptr<float[]> x(new float[(size_t)(n - 1) * ldx + 1]);
  for (size_t k = 0; k < (size_t)(n - 1) * ldx + 1; ++k) x[k] = k % ldx == 0 ? 1.0f : NAN;
  const size_t beta_size = sites ? (size_t)(sites - 1) * ldbeta + 1 : 0;
  std::unique_ptr<float[]> beta(new float[beta_size]);
  for (size_t k = 0; k < beta_size; ++k) beta[k] = k % ldbeta == 0 ? (float)(next_random() % 3) : NAN;
  const uint32_t rows = block.i_end - block.i_begin, cols = block.j_end - block.j_begin;
  const uint64_t ldo = cols + pad;
  const size_t out_size = (size_t)(rows - 1) * ldo + cols;
  std::unique_ptr<float[]> out(new float[out_size]);
  for (size_t k = 0; k < out_size; ++k) out[k] = -12345.0f;
  if (cuking_pcrelate_matrix_host(bits.get(), n, words, sites, x.get(), ldx, beta.get(), ldbeta, 1,
                                  0.01f, 0.99f, &block, out.get(), ldo) != CUKING_OK)
    return fail("refused", n, sites, pad);
  for (uint32_t i = 0; i < rows; ++i) {
    for (uint32_t j = 0; j < cols; ++j) {
      int64_t num = 0, count = 0;
      for (uint32_t s = 0; s < sites; ++s) {
        const int a = code[(size_t)(block.i_begin + i) * sites + s];
        const int b = code[(size_t)(block.j_begin + j) * sites + s];
        if (a == 3 || b == 3 || beta[(size_t)s * ldbeta] != 1.0f) continue;
        num += (a - 1) * (b - 1);
        ++count;
      }
      const float got = out[(size_t)i * ldo + j];
      if (count == 0 ? !std::isnan(got) : got != (float)num / (float)count)
        return fail("kin", n, sites, i * cols + j);
    }
    for (uint64_t c = cols; c < ldo && i + 1 < rows; ++c)
      if (out[(size_t)i * ldo + c] != -12345.0f) return fail("pad written", n, sites, pad);
  }
}

void check_helpers_and_refusals() {
  // the element functions against their definition, term by term
  for (int round = 0; round < 20000; ++round) {
    float xr[5], br[5];
    for (int c = 0; c < 5; ++c) {
      xr[c] = (float)((double)(next_random() % 2001) / 1000.0 - 1.0);
      br[c] = (float)((double)(next_random() % 2001) / 2000.0);
    }
    float acc = 0.0f;
    for (int c = 0; c < 5; ++c) acc = fmaf(xr[c], br[c], acc);
    const float mu = cuking::pcrelate_mu(xr, br, 5);
    if (mu != 0.5f * acc) return fail("pcrelate_mu", 0, 0, (uint32_t)round);
    const uint32_t code = (uint32_t)(next_random() & 3);
    float r, v;
    cuking::pcrelate_element(code, mu, 0.01f, 0.99f, &r, &v);
    const bool valid = code != 3 && 0.01f < mu && mu < 0.99f;
    if (valid != cuking::pcrelate_valid(code, mu, 0.01f, 0.99f)) return fail("valid", 0, 0, code);
    volatile float twice = 2.0f * mu, one_minus = 1.0f - mu;
    volatile float var = mu * one_minus;
    const float want_r = valid ? (float)code - twice : 0.0f;
    const float want_v = valid ? sqrtf(var) : 0.0f;
    if (r != want_r || v != want_v) return fail("pcrelate_element", 0, 0, code);
  }
  if (cuking::kPcrelateColumnsMax != CUKING_PCRELATE_COLUMNS_MAX ||
      !cuking::pcrelate_bounds_valid(0.0f, 1.0f) || cuking::pcrelate_bounds_valid(0.5f, 0.5f) ||
      cuking::pcrelate_bounds_valid(-0.1f, 0.5f) || cuking::pcrelate_bounds_valid(0.1f, 1.5f) ||
      cuking::pcrelate_bounds_valid(NAN, 0.5f) || cuking::pcrelate_bounds_valid(0.1f, NAN))
    fail("constants", 0, 0, 0);
  uint64_t bits[4] = {0, 0, 0, 0};  // two samples, one plane word: hom-ref everywhere
  float x[2] = {1, 1}, beta[2] = {1, 1}, out[4] = {9, 9, 9, 9};
  cuking_submatrix whole = {0, 2, 0, 2}, outside = {0, 3, 0, 3}, reversed = {2, 1, 2, 1};
  cuking_submatrix overlap = {0, 2, 1, 2}, empty = {1, 1, 0, 2};
  const cuking_status bad = CUKING_ERR_INVALID_ARGUMENT;
  // (r = -1, v = 0.5 at both sites: kin = 2 / (4 * 0.5) = 1)
  if (cuking_pcrelate_matrix_host(bits, 2, 2, 2, x, 1, beta, 1, 1, 0.01f, 0.99f, &whole, out, 2) !=
          CUKING_OK || out[0] != 1.0f || out[1] != 1.0f || out[2] != 1.0f || out[3] != 1.0f)
    fail("valid call", 2, 2, 1);
#define REFUSED(...) (cuking_pcrelate_matrix_host(__VA_ARGS__) != bad)
  if (REFUSED(nullptr, 2, 2, 2, x, 1, beta, 1, 1, 0.01f, 0.99f, &whole, out, 2) ||
      REFUSED(bits, 2, 2, 2, nullptr, 1, beta, 1, 1, 0.01f, 0.99f, &whole, out, 2) ||
      REFUSED(bits, 2, 2, 2, x, 1, nullptr, 1, 1, 0.01f, 0.99f, &whole, out, 2) ||
      REFUSED(bits, 2, 2, 2, x, 1, beta, 1, 1, 0.01f, 0.99f, &whole, nullptr, 2) ||
      REFUSED(bits, 2, 2, 2, x, 1, beta, 1, 1, 0.01f, 0.99f, nullptr, out, 2) ||
      REFUSED(bits, 2, 1, 2, x, 1, beta, 1, 1, 0.01f, 0.99f, &whole, out, 2) ||
      REFUSED(bits, 2, 0, 0, x, 1, beta, 1, 1, 0.01f, 0.99f, &whole, out, 2) ||
      REFUSED(bits, 2, 2, 65, x, 1, beta, 1, 1, 0.01f, 0.99f, &whole, out, 2) ||
      REFUSED(bits, 2, 2, 2, x, 1, beta, 1, 0, 0.01f, 0.99f, &whole, out, 2) ||
      REFUSED(bits, 2, 2, 2, x, 33, beta, 33, 33, 0.01f, 0.99f, &whole, out, 2) ||
      REFUSED(bits, 2, 2, 2, x, 1, beta, 2, 2, 0.01f, 0.99f, &whole, out, 2) ||
      REFUSED(bits, 2, 2, 2, x, 2, beta, 1, 2, 0.01f, 0.99f, &whole, out, 2) ||
      REFUSED(bits, 2, 2, 2, x, 1, beta, 1, 1, -0.01f, 0.99f, &whole, out, 2) ||
      REFUSED(bits, 2, 2, 2, x, 1, beta, 1, 1, 0.5f, 0.5f, &whole, out, 2) ||
      REFUSED(bits, 2, 2, 2, x, 1, beta, 1, 1, 0.01f, 1.01f, &whole, out, 2) ||
      REFUSED(bits, 2, 2, 2, x, 1, beta, 1, 1, NAN, 0.99f, &whole, out, 2) ||
      REFUSED(bits, 2, 2, 2, x, 1, beta, 1, 1, 0.01f, 0.99f, &outside, out, 3) ||
      REFUSED(bits, 2, 2, 2, x, 1, beta, 1, 1, 0.01f, 0.99f, &reversed, out, 2) ||
      REFUSED(bits, 2, 2, 2, x, 1, beta, 1, 1, 0.01f, 0.99f, &overlap, out, 2) ||
      REFUSED(bits, 2, 2, 2, x, 1, beta, 1, 1, 0.01f, 0.99f, &whole, out, 1))
    fail("refusals", 2, 2, 1);
#undef REFUSED
  if (out[0] != 1.0f || out[1] != 1.0f || out[2] != 1.0f || out[3] != 1.0f)
    fail("a refused call wrote", 2, 2, 1);
  out[0] = out[1] = out[2] = out[3] = 9;
  if (cuking_pcrelate_matrix_host(nullptr, 2, 2, 2, nullptr, 1, nullptr, 1, 1, 0.01f, 0.99f, &empty,
                                  nullptr, 2) != CUKING_OK ||
      cuking_pcrelate_matrix_host(nullptr, 2, 2, 0, nullptr, 1, nullptr, 1, 1, 0.01f, 0.99f, &whole,
                                  out, 2) != CUKING_OK ||
      !std::isnan(out[0]) || !std::isnan(out[1]) || !std::isnan(out[2]) || !std::isnan(out[3]))
    fail("calls without work", 0, 0, 1);
}

}  // namespace

int main() {
  const uint32_t samples[] = {1, 33, 130}, sites[] = {0, 1, 63, 64, 65, 700};
  for (const uint32_t n : samples)
    for (const uint32_t s : sites)
      for (const uint32_t pad : {0u, 3u}) {
        run_shape(n, s, {0, n, 0, n}, pad);
        if (n >= 33) run_shape(n, s, {5, 20, 21, n}, pad);
        run_shape(n, s, {n - 1, n, n - 1, n}, pad);
      }
  check_helpers_and_refusals();
  printf("%d failures\n", g_failures);
  return g_failures != 0;
}
