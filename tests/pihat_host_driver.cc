// Stand-alone driver of the PI_HAT host twins for the sanitizer build of tests/test_pihat_host.py
// (built and run by tests/host_driver.py, csrc/king_host.cc linked in): a program of its own,
// nothing is loaded into Python.
//
// Standard input: "R T", then R count rows "hom_ref het hom_var", then T triples "ibs0 ibs1
// ibs2".  Prints "model" with the bits of the five expectations in hex and sites_used
// (cuking_pihat_model_host), then for the bounded and the unbounded form one line "z" per triple
// with the bits of z0, z1, z2, pi_hat (cuking_pihat_records_host), checked here against
// pihat_z_of_counts (csrc/king_pihat.h) directly.  Then a random block through
// cuking_compute_pihat_host -- buffers are heap blocks of exactly the size the contract names, so
// a store past max_results is a sanitizer report -- and the refusals.  Ends with "<n> failures".
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "cuking_amd.h"
#include "host_driver_common.h"
#include "king_pihat.h"

static uint64_t bits_of(double x) {
  uint64_t b;
  std::memcpy(&b, &x, sizeof b);
  return b;
}

int main() {
  unsigned long long R = 0, T = 0, a, b, c;
  if (std::scanf("%llu %llu", &R, &T) != 2) return 2;
  uint32_t *counts = new uint32_t[(size_t)R * 4];
  for (uint32_t s = 0; s < R; ++s) {
    if (std::scanf("%llu %llu %llu", &a, &b, &c) != 3) return 2;
    counts[4 * s + 0] = (uint32_t)a;
    counts[4 * s + 1] = (uint32_t)b;
    counts[4 * s + 2] = (uint32_t)c;
    counts[4 * s + 3] = 0xDEADBEEFu + s;  // missing: ignored
  }
  cuking_result *recs = new cuking_result[T];
  for (uint32_t k = 0; k < T; ++k) {
    if (std::scanf("%llu %llu %llu", &a, &b, &c) != 3) return 2;
    recs[k] = cuking_result{k, k + 1, -1.f, (uint32_t)a, (uint32_t)b, (uint32_t)c};
  }
  cuking_pihat_model model;
  expect("model", cuking_pihat_model_host(counts, (uint32_t)R, &model), CUKING_OK);
  std::printf("model %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64
              " %u\n", bits_of(model.e00), bits_of(model.e01), bits_of(model.e02),
              bits_of(model.e11), bits_of(model.e12), model.sites_used);
  double *z = new double[(size_t)T * 4];
  for (int unbounded = 0; unbounded < 2; ++unbounded) {
    expect("records",
           cuking_pihat_records_host(recs, T, &model, unbounded ? CUKING_PIHAT_UNBOUNDED : 0u, z),
           CUKING_OK);
    for (uint32_t k = 0; k < T; ++k) {
      double d[4];
      cuking::pihat_z_of_counts(model.e00, model.e01, model.e02, model.e11, model.e12,
                                recs[k].ibs0, recs[k].ibs1, recs[k].ibs2, !unbounded, d);
      for (int q = 0; q < 4; ++q)
        if (bits_of(d[q]) != bits_of(z[4 * k + q])) fail("records differ", k, q, unbounded);
      std::printf("z %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n",
                  bits_of(z[4 * k]), bits_of(z[4 * k + 1]), bits_of(z[4 * k + 2]),
                  bits_of(z[4 * k + 3]));
    }
  }

  // a random block: 37 samples x 200 sites (4 plane words, the last 56 sites missing)
  const uint32_t n = 37, sites = 200, wps = 8, plane = wps / 2;
  uint64_t *bit_sets = new uint64_t[(size_t)n * wps];
  for (uint32_t s = 0; s < n; ++s) {
    uint64_t *row = bit_sets + (size_t)s * wps;
    for (uint32_t k = 0; k < 64 * plane; ++k) {
      const uint32_t r = (uint32_t)(next_random() % 100);
      set_code(row, plane, k, k >= sites || r < 3 ? 3u : r < 50 ? 0u : r < 80 ? 1u : 2u);
    }
  }
  const cuking_pihat_model m2 = {0.08, 0.42, 0.5, 0.36, 0.64, sites};
  cuking_submatrix blocks[2];
  cuking_submatrix_init(&blocks[0], n, 1, 0);
  cuking_submatrix_init(&blocks[1], n, 2, 1);  // off-diagonal: rows [0, 19) x columns [19, 37)
  for (const cuking_submatrix &sm : blocks) {
    uint32_t total = 0, again = 0;
    // (max_results = 0 counts: the count is there, the status says it does not fit)
    expect("count", cuking_compute_pihat_host(&sm, wps, bit_sets, &m2, -1.f, 0, 0, nullptr, &total),
           CUKING_ERR_RESOURCE_EXHAUSTED);
    if (total != cuking_submatrix_num_pairs(&sm)) fail("every pair qualifies at -1", total);
    cuking_result *all = new cuking_result[total];
    expect("exact", cuking_compute_pihat_host(&sm, wps, bit_sets, &m2, -1.f, 0, total, all, &again),
           CUKING_OK);
    if (again != total) fail("count of the exact call", again, total);
    for (uint32_t k = 0; k < total; ++k) {
      if (!(all[k].sample_i < all[k].sample_j)) fail("sample order", k);
      if (all[k].kin != cuking::pihat_of_counts(m2.e00, m2.e01, m2.e02, m2.e11, m2.e12,
                                                all[k].ibs0, all[k].ibs1, all[k].ibs2, 0))
        fail("kin is not pihat_of_counts", k);
      if (all[k].ibs0 + all[k].ibs1 + all[k].ibs2 > sites) fail("counts beyond the sites", k);
    }
    cuking_result *shorter = new cuking_result[total - 1];
    expect("one short",
           cuking_compute_pihat_host(&sm, wps, bit_sets, &m2, -1.f, 0, total - 1, shorter, &again),
           CUKING_ERR_RESOURCE_EXHAUSTED);
    if (again != total || std::memcmp(shorter, all, (size_t)(total - 1) * sizeof *all) != 0)
      fail("one short: count or records", again, total);
    delete[] shorter;
    delete[] all;
  }

  // refusals, and what is no work
  uint32_t num = 7;
  expect("flags", cuking_pihat_records_host(recs, T, &model, 2, z), CUKING_ERR_INVALID_ARGUMENT);
  expect("null model", cuking_pihat_records_host(recs, T, nullptr, 0, z),
         CUKING_ERR_INVALID_ARGUMENT);
  expect("no records", cuking_pihat_records_host(nullptr, 0, &model, 0, nullptr), CUKING_OK);
  expect("null counts", cuking_pihat_model_host(nullptr, 1, &model), CUKING_ERR_INVALID_ARGUMENT);
  expect("null num", cuking_compute_pihat_host(&blocks[0], wps, bit_sets, &m2, 0.f, 0, 0, nullptr,
                                               nullptr), CUKING_ERR_INVALID_ARGUMENT);
  expect("odd words", cuking_compute_pihat_host(&blocks[0], 7, bit_sets, &m2, 0.f, 0, 0, nullptr,
                                                &num), CUKING_ERR_INVALID_ARGUMENT);
  if (num != 0) fail("a refused call zeroes the count", num);

  delete[] bit_sets;
  delete[] z;
  delete[] recs;
  delete[] counts;
  std::printf("%d failures\n", g_failures);
  return g_failures != 0;
}
