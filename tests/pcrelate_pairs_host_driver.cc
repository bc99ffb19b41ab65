// Stand-alone driver of the host side of PC-Relate for listed pairs for the sanitizer build of
// tests/test_pcrelate_pairs_host.py (built and run by tests/host_driver.py, csrc/king_host.cc
// linked in).  Every buffer is an exact-size heap allocation, so a byte read or written past
// an end is caught.
//   1. cuking_pcrelate_pairs_host in the exact setting (d = 1, X = 1, beta in {0, 1, 2}, f null:
//      every sum a dyadic number) against the integer formula on plain code arrays, strides 8 and
//      24 (the last entry cut off after its two indices), pitches equal to and above the need,
//      garbage bits beyond num_sites, self pairs, swapped pairs and indices out of range;
//   2. the same with f given; the refusals; the calls without work.
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

bool same_float(float a, float b) { return (std::isnan(a) && std::isnan(b)) || a == b; }

void run_shape(uint32_t n, uint32_t sites, uint32_t num_pairs, uint32_t stride, uint32_t pad,
               bool with_f) {
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
  // f = 1 for everybody doubles s2: 16 dden = 4 n and e = dom - 1/2 (0 for hom, -1/2 for het)
  std::unique_ptr<float[]> f(new float[n]);
  for (uint32_t i = 0; i < n; ++i) f[i] = 1.0f;
  // the list: exactly (num_pairs - 1) * stride + 8 bytes
  const size_t list_bytes = (size_t)(num_pairs - 1) * stride + 8;
  std::unique_ptr<unsigned char[]> list(new unsigned char[list_bytes]);
  for (size_t k = 0; k < list_bytes; ++k) list[k] = (unsigned char)next_random();
  std::vector<uint32_t> index(2 * (size_t)num_pairs);
  for (uint32_t p = 0; p < num_pairs; ++p) {
    uint32_t i = (uint32_t)(next_random() % n), j = (uint32_t)(next_random() % n);
    if (p % 7 == 3) j = i;                              // a self pair
    if (p % 11 == 5) j = n + (uint32_t)(next_random() % 3);   // out of range
    if (p % 13 == 6) i = 0xFFFFFFFFu;
    index[2 * p] = i;
    index[2 * p + 1] = j;
    memcpy(list.get() + (size_t)p * stride, &index[2 * p], 8);
  }
  std::unique_ptr<cuking_pcrelate_pair[]> out(new cuking_pcrelate_pair[num_pairs]);
  if (cuking_pcrelate_pairs_host(bits.get(), n, words, sites, x.get(), ldx, beta.get(), ldbeta, 1,
                                 0.01f, 0.99f, with_f ? f.get() : nullptr, list.get(), num_pairs,
                                 stride, out.get()) != CUKING_OK)
    return fail("refused", n, sites, stride);
  for (uint32_t p = 0; p < num_pairs; ++p) {
    const uint32_t i = index[2 * p], j = index[2 * p + 1];
    int64_t num = 0, count = 0, zyg = 0, both_het = 0, ibs0 = 0;
    if (i < n && j < n)
      for (uint32_t s = 0; s < sites; ++s) {
        const int a = code[(size_t)i * sites + s], b = code[(size_t)j * sites + s];
        if (a == 3 || b == 3 || beta[(size_t)s * ldbeta] != 1.0f) continue;
        num += (a - 1) * (b - 1);
        ++count;
        zyg += ((a == 1) == (b == 1)) ? 1 : -1;
        both_het += (a == 1 && b == 1) ? 1 : 0;   // (with f = 1: e_i e_j = 1/4 for het x het)
        ibs0 += ((a ^ b) == 2) ? 1 : 0;
      }
    const float kin = (float)num / (float)count;
    const float k2 = with_f ? (float)both_het / (float)count : (float)zyg / (float)count;
    const float high = (1.0f - 4.0f * kin) + k2;
    const float low = (float)ibs0 / ((float)count / 8.0f);
    const float k0 = kin > CUKING_PCRELATE_K0_SWITCH ? high : low;
    const float k1 = (1.0f - k2) - k0;
    const cuking_pcrelate_pair &got = out[p];
    if (got.sample_i != i || got.sample_j != j || got.ibs0 != (uint32_t)ibs0 ||
        got.sites != (uint32_t)count || !same_float(got.kin, kin) || !same_float(got.k0, k0) ||
        !same_float(got.k1, k1) || !same_float(got.k2, k2))
      return fail("row", n, sites, p);
    if (count == 0 && !(std::isnan(got.kin) && std::isnan(got.k0) && std::isnan(got.k1) &&
                        std::isnan(got.k2)))
      return fail("a pair without a site", n, sites, p);
  }
}

void check_refusals() {
  if (cuking::kPcrelateK0Switch != CUKING_PCRELATE_K0_SWITCH || sizeof(cuking_pcrelate_pair) != 32 ||
      cuking::pcrelate_pair_stride_valid(4) || cuking::pcrelate_pair_stride_valid(10) ||
      !cuking::pcrelate_pair_stride_valid(8) || !cuking::pcrelate_pair_stride_valid(24))
    fail("constants", 0, 0, 0);
  uint64_t bits[4] = {0, 0, 0, 0};  // two samples, one plane word: hom-ref everywhere
  float x[2] = {1, 1}, beta[2] = {1, 1};
  uint32_t pairs[4] = {0, 1, 1, 1};
  cuking_pcrelate_pair out[2];
  memset(out, 0x5A, sizeof(out));
  cuking_pcrelate_pair before[2];
  memcpy(before, out, sizeof(out));
  const cuking_status bad = CUKING_ERR_INVALID_ARGUMENT;
#define REFUSED(...) (cuking_pcrelate_pairs_host(__VA_ARGS__) != bad)
  if (REFUSED(nullptr, 2, 2, 2, x, 1, beta, 1, 1, 0.01f, 0.99f, nullptr, pairs, 2, 8, out) ||
      REFUSED(bits, 2, 2, 2, nullptr, 1, beta, 1, 1, 0.01f, 0.99f, nullptr, pairs, 2, 8, out) ||
      REFUSED(bits, 2, 2, 2, x, 1, nullptr, 1, 1, 0.01f, 0.99f, nullptr, pairs, 2, 8, out) ||
      REFUSED(bits, 2, 2, 2, x, 1, beta, 1, 1, 0.01f, 0.99f, nullptr, nullptr, 2, 8, out) ||
      REFUSED(bits, 2, 2, 2, x, 1, beta, 1, 1, 0.01f, 0.99f, nullptr, pairs, 2, 8, nullptr) ||
      REFUSED(bits, 2, 1, 2, x, 1, beta, 1, 1, 0.01f, 0.99f, nullptr, pairs, 2, 8, out) ||
      REFUSED(bits, 2, 0, 0, x, 1, beta, 1, 1, 0.01f, 0.99f, nullptr, pairs, 2, 8, out) ||
      REFUSED(bits, 2, 2, 65, x, 1, beta, 1, 1, 0.01f, 0.99f, nullptr, pairs, 2, 8, out) ||
      REFUSED(bits, 2, 2, 2, x, 1, beta, 1, 0, 0.01f, 0.99f, nullptr, pairs, 2, 8, out) ||
      REFUSED(bits, 2, 2, 2, x, 33, beta, 33, 33, 0.01f, 0.99f, nullptr, pairs, 2, 8, out) ||
      REFUSED(bits, 2, 2, 2, x, 1, beta, 2, 2, 0.01f, 0.99f, nullptr, pairs, 2, 8, out) ||
      REFUSED(bits, 2, 2, 2, x, 2, beta, 1, 2, 0.01f, 0.99f, nullptr, pairs, 2, 8, out) ||
      REFUSED(bits, 2, 2, 2, x, 1, beta, 1, 1, -0.01f, 0.99f, nullptr, pairs, 2, 8, out) ||
      REFUSED(bits, 2, 2, 2, x, 1, beta, 1, 1, 0.5f, 0.5f, nullptr, pairs, 2, 8, out) ||
      REFUSED(bits, 2, 2, 2, x, 1, beta, 1, 1, 0.01f, 1.01f, nullptr, pairs, 2, 8, out) ||
      REFUSED(bits, 2, 2, 2, x, 1, beta, 1, 1, NAN, 0.99f, nullptr, pairs, 2, 8, out) ||
      REFUSED(bits, 2, 2, 2, x, 1, beta, 1, 1, 0.01f, 0.99f, nullptr, pairs, 2, 0, out) ||
      REFUSED(bits, 2, 2, 2, x, 1, beta, 1, 1, 0.01f, 0.99f, nullptr, pairs, 2, 4, out) ||
      REFUSED(bits, 2, 2, 2, x, 1, beta, 1, 1, 0.01f, 0.99f, nullptr, pairs, 2, 10, out) ||
      REFUSED(bits, 2, 2, 2, x, 1, beta, 1, 1, 0.01f, 0.99f, nullptr, pairs, 0, 6, nullptr))
    fail("refusals", 2, 2, 1);
#undef REFUSED
  if (memcmp(before, out, sizeof(out)) != 0) fail("a refused call wrote", 2, 2, 1);
  // (hom-ref at mu = 1/2 at both sites: r = -1, v = 1/2, e = 1/4, s2 = 1/4, a = b = 1/4)
  if (cuking_pcrelate_pairs_host(bits, 2, 2, 2, x, 1, beta, 1, 1, 0.01f, 0.99f, nullptr, pairs, 2,
                                 8, out) != CUKING_OK ||
      out[0].kin != 1.0f || out[0].k2 != 1.0f || out[0].k0 != -2.0f || out[0].k1 != 2.0f ||
      out[0].sites != 2 || out[0].ibs0 != 0 || out[1].sample_i != 1 || out[1].kin != 1.0f)
    fail("valid call", 2, 2, 1);
  memcpy(out, before, sizeof(out));
  if (cuking_pcrelate_pairs_host(nullptr, 2, 2, 2, nullptr, 1, nullptr, 1, 1, 0.01f, 0.99f, nullptr,
                                 nullptr, 0, 8, nullptr) != CUKING_OK ||
      memcmp(before, out, sizeof(out)) != 0 ||
      cuking_pcrelate_pairs_host(nullptr, 2, 2, 0, nullptr, 1, nullptr, 1, 1, 0.01f, 0.99f, nullptr,
                                 pairs, 2, 8, out) != CUKING_OK ||
      !std::isnan(out[0].kin) || !std::isnan(out[1].k1) || out[0].sites != 0 ||
      out[1].sample_j != 1)
    fail("calls without work", 0, 0, 1);
}

}  // namespace

int main() {
  const uint32_t samples[] = {1, 33}, sites[] = {0, 1, 63, 64, 65, 700}, pairs[] = {1, 65};
  for (const uint32_t n : samples)
    for (const uint32_t s : sites)
      for (const uint32_t p : pairs)
        for (const uint32_t stride : {8u, 24u})
          for (const uint32_t pad : {0u, 3u}) {
            run_shape(n, s, p, stride, pad, false);
            run_shape(n, s, p, stride, pad, true);
          }
  check_refusals();
  printf("%d failures\n", g_failures);
  return g_failures != 0;
}
