// Stand-alone driver of cuking_pack_bed_host for the sanitizer build of
// tests/test_bed_host.py (built and run by tests/host_driver.py, csrc/king_host.cc linked in):
// 37 samples x 129 sites, every shard of a split factor of 3, one-shot and in chunks, every
// buffer an exact-size heap allocation so that a byte read or written past an end is caught.
// The result is compared with cuking_pack_host of the same genotypes as triples.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "cuking_amd.h"
#include "host_driver_common.h"

int main() {
  const uint32_t N = 37, M = 129;
  const uint64_t row_bytes = cuking_bed_row_bytes(N);
  const uint32_t wps = cuking_words_per_sample(M);
  std::unique_ptr<uint8_t[]> rows(new uint8_t[M * row_bytes]);
  for (uint64_t k = 0; k < M * row_bytes; ++k) {
    next_random();
    rows[k] = (uint8_t)(g_state >> 56);  // (the top byte of the generator's state)
  }
  // the same genotypes as triples (code 1 = missing = no triple)
  std::vector<int64_t> row_idx, col_idx;
  std::vector<int32_t> n_alt;
  const int32_t alt_of_code[4] = {2, -1, 1, 0};
  for (uint32_t site = 0; site < M; ++site)
    for (uint32_t s = 0; s < N; ++s) {
      const int32_t alt = alt_of_code[(rows[site * row_bytes + (s >> 2)] >> (2 * (s & 3))) & 3];
      if (alt < 0) continue;
      row_idx.push_back(site);
      col_idx.push_back(s);
      n_alt.push_back(alt);
    }
  for (uint32_t shard = 0; shard < 6; ++shard) {
    cuking_submatrix sm;
    if (cuking_submatrix_init(&sm, N, 3, shard) != CUKING_OK) return 2;
    const size_t words = (size_t)cuking_submatrix_num_samples(&sm) * wps;
    std::unique_ptr<uint64_t[]> want(new uint64_t[words]), got(new uint64_t[words]);
    memset(want.get(), 0xFF, words * 8);
    if (cuking_pack_host(&sm, wps, want.get(), row_idx.data(), col_idx.data(), n_alt.data(),
                         n_alt.size()) != CUKING_OK)
      return 2;
    for (int chunked = 0; chunked < 2; ++chunked) {
      memset(got.get(), 0xA5, words * 8);
      cuking_status st = CUKING_OK;
      if (!chunked) {
        st = cuking_pack_bed_host(&sm, wps, got.get(), rows.get(), row_bytes, 0, M, M);
      } else {
        // (each chunk gets a copy of exactly its rows: nothing outside them may be read)
        const uint32_t cuts[4] = {0, 64, 128, M};
        for (int c = 0; c < 3 && st == CUKING_OK; ++c) {
          const size_t bytes = (size_t)(cuts[c + 1] - cuts[c]) * row_bytes;
          std::unique_ptr<uint8_t[]> part(new uint8_t[bytes]);
          memcpy(part.get(), rows.get() + cuts[c] * row_bytes, bytes);
          st = cuking_pack_bed_host(&sm, wps, got.get(), part.get(), row_bytes, cuts[c],
                                    cuts[c + 1], M);
        }
      }
      if (st != CUKING_OK) {
        fprintf(stderr, "shard %u: %s\n", shard, cuking_last_error());
        ++g_failures;
      } else if (memcmp(want.get(), got.get(), words * 8) != 0) {
        fprintf(stderr, "shard %u (%s): differs from cuking_pack_host\n", shard,
                chunked ? "chunks" : "one call");
        ++g_failures;
      }
    }
  }
  printf("bed_host_driver: %d failures\n", g_failures);
  return g_failures != 0;
}
