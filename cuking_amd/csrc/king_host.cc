// Host-only half of the C ABI (include/cuking_amd.h): Submatrix arithmetic,
// bitset sizing, the host pack with its relaxed atomics, the narrowing step of
// the device pack, the PLINK .bed pack and its checks, the record sort, the
// per-thread error message.  Plain C++ (no HIP): hipcc compiles it into
// libcuking_amd.so, and the sanitizer tests compile the same file with g++
// -fsanitize=thread / address so that the code that runs on many reader threads
// is instrumented (tests/test_cli.py, tests/test_bed_host.py).
#include "king_host.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <string>
#include <tuple>
#include <vector>

#include "../host/schedule.h"
#include "king_submatrix.h"
#include "king_geno.h"
#include "king_hwe.h"
#include "king_ibd.h"
#include "king_kin_summary.h"
#include "king_ld.h"
#include "king_mendel.h"
#include "king_pcrelate.h"
#include "king_pihat.h"
#include "king_unrelated.h"

using namespace cuking;

namespace {

thread_local std::string g_last_error;

uint32_t ceil_div(uint32_t a, uint32_t b) {
  return (uint32_t)(((uint64_t)a + b - 1) / b);
}
uint32_t round_up(uint32_t a, uint32_t b) { return ceil_div(a, b) * b; }

}  // namespace

cuking_status cuking_fail(cuking_status code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return code;
}

cuking_status cuking_check_block(const cuking_submatrix *sm,
                          uint32_t words_per_sample) {
  if (sm == nullptr) return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null submatrix");
  if (sm->i_end < sm->i_begin || sm->j_end < sm->j_begin)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "submatrix ranges are reversed: rows [%u, %u) x columns [%u, %u)",
                       sm->i_begin, sm->i_end, sm->j_begin, sm->j_end);
  if (!sm_is_diag(*sm) && sm->j_begin < sm->i_end && sm_num_rows(*sm) != 0 &&
      sm_num_cols(*sm) != 0)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                "row and column ranges must be identical or disjoint with "
                "rows first");
  if (sm_is_diag(*sm) && sm->i_end != sm->j_end)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                "a diagonal block needs identical row and column ranges");
  if (words_per_sample == 0 || (words_per_sample & 1))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                "words_per_sample (%u) must be a positive even number", words_per_sample);
  return CUKING_OK;
}

extern "C" {

const char *cuking_last_error(void) { return g_last_error.c_str(); }
uint32_t cuking_abi_version(void) { return CUKING_ABI_VERSION; }

// ---- host-only helpers ----------------------------------------------------

cuking_status cuking_submatrix_init(cuking_submatrix *sm, uint32_t num_samples,
                                    uint32_t split_factor,
                                    uint32_t shard_index) {
  if (sm == nullptr) return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null submatrix");
  if (split_factor == 0)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "Invalid split factor");
  const uint64_t shards = (uint64_t)split_factor * ((uint64_t)split_factor + 1) / 2;
  if (shard_index >= shards)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "Invalid shard index");
  // Row r of the block triangle starts at shard r*k - r(r-1)/2.
  uint32_t block_i = 0;
  uint64_t first = 0;
  while (first + (split_factor - block_i) <= shard_index) {
    first += split_factor - block_i;
    ++block_i;
  }
  const uint32_t block_j = block_i + (uint32_t)(shard_index - first);
  const uint64_t size = ceil_div(num_samples, split_factor);
  auto clamp = [&](uint64_t x) {
    return (uint32_t)std::min<uint64_t>(x, num_samples);
  };
  sm->i_begin = clamp(block_i * size);
  sm->i_end = clamp(block_i * size + size);
  sm->j_begin = clamp(block_j * size);
  sm->j_end = clamp(block_j * size + size);
  return CUKING_OK;
}

uint32_t cuking_submatrix_num_rows(const cuking_submatrix *sm) { return sm_num_rows(*sm); }
uint32_t cuking_submatrix_num_cols(const cuking_submatrix *sm) { return sm_num_cols(*sm); }
uint32_t cuking_submatrix_num_samples(const cuking_submatrix *sm) { return sm_num_samples(*sm); }
uint32_t cuking_submatrix_contains(const cuking_submatrix *sm, uint32_t index) {
  return sm_contains(*sm, index) ? 1u : 0u;
}
uint32_t cuking_submatrix_sample_offset(const cuking_submatrix *sm, uint32_t index) {
  return sm_sample_offset(*sm, index);
}

uint64_t cuking_submatrix_num_pairs(const cuking_submatrix *sm) {
  const uint64_t r = sm_num_rows(*sm), c = sm_num_cols(*sm);
  if (sm_is_diag(*sm)) return r * (r - (r ? 1 : 0)) / 2;
  // Off-diagonal blocks lie strictly above the diagonal: every (i, j) counts.
  uint64_t n = 0;
  if (sm->j_begin >= sm->i_end) return r * c;
  for (uint32_t i = sm->i_begin; i < sm->i_end; ++i) {
    const uint32_t lo = std::max(sm->j_begin, i + 1);
    if (lo < sm->j_end) n += sm->j_end - lo;
  }
  return n;
}

uint32_t cuking_padded_sites(uint32_t num_sites) { return round_up(num_sites, 32u); }
uint32_t cuking_words_per_sample(uint32_t num_sites) {
  return 2u * ceil_div(cuking_padded_sites(num_sites), 64u);
}
uint64_t cuking_bytes_per_pair(uint32_t words_per_sample) {
  return 2ull * words_per_sample * sizeof(uint64_t);
}

namespace {

// Per reader thread: the AND masks of ONE 64-site word column, per stored sample.
// Input tables are site-major (the Spark writer's order, mt_to_cuking_inputs.py:24-34:
// all samples of a site, then the next site), so consecutive triples fall into the
// same word of different samples' planes: 64 sites x n samples of them per column.
// Collecting their bits here and clearing each (sample, plane) word once replaces
// ~32 atomic read-modify-writes per word (15 ns per triple, most of the host
// pack's time) by one.
struct WordColumn {
  std::vector<uint64_t> het, hom;   // bits to KEEP (all ones = untouched)
  std::vector<uint8_t> dirty;
  std::vector<uint32_t> touched;    // samples with dirty != 0, in arrival order
  void Reserve(uint32_t samples) {
    if (het.size() < samples) {
      het.resize(samples, ~0ull);
      hom.resize(samples, ~0ull);
      dirty.resize(samples, 0);
    }
  }
};

}  // namespace

cuking_status cuking_pack_host(const cuking_submatrix *sm,
                               uint32_t words_per_sample, uint64_t *bit_set,
                               const int64_t *row_idx, const int64_t *col_idx,
                               const int32_t *n_alt_alleles,
                               size_t num_triples) {
  cuking_status st = cuking_check_block(sm, words_per_sample);
  if (st != CUKING_OK) return st;
  const uint32_t plane_words = words_per_sample / 2;
  const uint64_t plane_bits = (uint64_t)plane_words * 64;
  auto clear_bit = [](uint64_t *plane, uint64_t index) {
    __atomic_and_fetch(plane + (index >> 6), ~(1ull << (index & 63)),
                       __ATOMIC_RELAXED);
  };
  // cuking.cu:675-703 per triple; `direct` = straight into the bitset (one atomic AND
  // per bit, cuking.cu:317-323), otherwise through the word column.
  thread_local WordColumn wc_of_thread;
  WordColumn &wc = wc_of_thread;  // (one thread-local lookup per call, not per triple)
  // (short calls, and tables that are not site-major -- detected below -- go direct)
  bool direct = num_triples < 1024;
  if (!direct) wc.Reserve(cuking_submatrix_num_samples(sm));
  uint64_t *const keep_het = wc.het.data(), *const keep_hom = wc.hom.data();
  uint8_t *const dirty = wc.dirty.data();
  uint64_t column = ~0ull;      // word index the masks belong to
  size_t flushes = 0;
  auto flush = [&]() {
    for (const uint32_t s : wc.touched) {
      uint64_t *het = bit_set + (uint64_t)s * words_per_sample + column;
      if (keep_het[s] != ~0ull) __atomic_and_fetch(het, keep_het[s], __ATOMIC_RELAXED);
      if (keep_hom[s] != ~0ull) __atomic_and_fetch(het + plane_words, keep_hom[s], __ATOMIC_RELAXED);
      keep_het[s] = keep_hom[s] = ~0ull;
      dirty[s] = 0;
    }
    wc.touched.clear();
    ++flushes;
  };
  for (size_t t = 0; t < num_triples; ++t) {
    const int64_t col = col_idx[t];
    if (col < 0 || col > 0xFFFFFFFFll || !sm_contains(*sm, (uint32_t)col))
      continue;
    const int64_t row = row_idx[t];
    if (row < 0 || (uint64_t)row >= plane_bits) {
      if (!direct) flush();
      return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                  "row_idx %lld outside the %llu padded sites", (long long)row,
                  (unsigned long long)plane_bits);
    }
    const int32_t alt = n_alt_alleles[t];
    if (alt < 0 || alt > 2) {
      if (!direct) flush();
      return cuking_fail(CUKING_ERR_FAILED_PRECONDITION,
                  "Invalid value for n_alt_alleles (%d) encountered", alt);
    }
    const uint32_t sample = sm_sample_offset(*sm, (uint32_t)col);
    if (direct) {
      uint64_t *het = bit_set + (uint64_t)sample * words_per_sample;
      if (alt != 1) clear_bit(het, (uint64_t)row);                // 0 and 2: not het
      if (alt != 2) clear_bit(het + plane_words, (uint64_t)row);  // 0 and 1: not hom-alt
      continue;
    }
    const uint64_t w = (uint64_t)row >> 6;
    if (w != column) {
      if (!wc.touched.empty()) flush();
      column = w;
      // Not site-major after all (a column change every few triples): the masks
      // buy nothing, the rest of the call goes direct.
      if (flushes >= 256 && t < 8 * flushes) {
        direct = true;
        --t;  // this triple again, on the direct path
        continue;
      }
    }
    if (!dirty[sample]) {
      dirty[sample] = 1;
      wc.touched.push_back(sample);
    }
    // (branch-free: a mask of all ones where the plane keeps its bit)
    const uint64_t bit = 1ull << (row & 63);
    keep_het[sample] &= ~(alt != 1 ? bit : 0ull);
    keep_hom[sample] &= ~(alt != 2 ? bit : 0ull);
  }
  if (!direct && !wc.touched.empty()) flush();
  return CUKING_OK;
}

cuking_status cuking_narrow_triples(const cuking_submatrix *sm, uint32_t words_per_sample,
                                    const int64_t *row_idx, const int64_t *col_idx,
                                    const int32_t *n_alt_alleles, size_t num_triples,
                                    uint32_t *site, uint32_t *sample_alt,
                                    size_t *num_out) {
  cuking_status st = cuking_check_block(sm, words_per_sample);
  if (st != CUKING_OK) return st;
  if (num_out == nullptr) return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null out pointer");
  *num_out = 0;
  if (cuking_submatrix_num_samples(sm) > 0x3FFFFFFFu)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "block holds more than 2^30 samples");
  const uint64_t plane_bits = (uint64_t)(words_per_sample / 2) * 64;
  size_t w = 0;
  for (size_t t = 0; t < num_triples; ++t) {
    const int64_t col = col_idx[t];
    if (col < 0 || col > 0xFFFFFFFFll || !sm_contains(*sm, (uint32_t)col)) continue;
    const int64_t row = row_idx[t];
    if (row < 0 || (uint64_t)row >= plane_bits)
      return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                  "row_idx %lld outside the %llu padded sites", (long long)row,
                  (unsigned long long)plane_bits);
    const int32_t g = n_alt_alleles[t];
    if (g < 0 || g > 2)
      return cuking_fail(CUKING_ERR_FAILED_PRECONDITION,
                  "Invalid value for n_alt_alleles (%d) encountered", g);
    site[w] = (uint32_t)row;
    sample_alt[w] = sm_sample_offset(*sm, (uint32_t)col) | ((uint32_t)g << 30);
    ++w;
  }
  *num_out = w;
  return CUKING_OK;
}

// ---- PLINK .bed input: the format's arithmetic, the checks and the host pack ----------------
uint64_t cuking_bed_row_bytes(uint32_t num_samples_total) {
  return ((uint64_t)num_samples_total + 3) / 4;
}

cuking_status cuking_bed_check(const uint8_t magic[3], uint64_t file_bytes,
                               uint32_t num_samples_total, uint32_t num_sites) {
  if (magic == nullptr) return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null magic pointer");
  if (magic[0] != 0x6c || magic[1] != 0x1b)
    return cuking_fail(CUKING_ERR_FAILED_PRECONDITION,
                       "not a PLINK .bed file: it starts with %02x %02x, not 6c 1b", magic[0],
                       magic[1]);
  if (magic[2] == 0x00)
    return cuking_fail(CUKING_ERR_FAILED_PRECONDITION,
                       "a sample-major .bed (third byte 00) is not supported: rewrite it "
                       "variant-major (third byte 01)");
  if (magic[2] != 0x01)
    return cuking_fail(CUKING_ERR_FAILED_PRECONDITION,
                       "not a PLINK .bed file: its third byte is %02x, not 01", magic[2]);
  const uint64_t need = 3 + (uint64_t)num_sites * cuking_bed_row_bytes(num_samples_total);
  if (file_bytes != need)
    return cuking_fail(CUKING_ERR_FAILED_PRECONDITION,
                       "the .bed file holds %llu bytes, but %u samples (.fam) x %u sites (.bim) "
                       "need %llu: truncated, or not the .bed of these two files",
                       (unsigned long long)file_bytes, num_samples_total, num_sites,
                       (unsigned long long)need);
  return CUKING_OK;
}

}  // extern "C"

cuking_status cuking_check_bed_args(const cuking_submatrix *sm, uint32_t words_per_sample,
                                    const void *bit_set, const void *bed_rows,
                                    uint64_t row_bytes, uint32_t site_begin, uint32_t site_end,
                                    uint32_t num_sites) {
  if (sm == nullptr || bit_set == nullptr || bed_rows == nullptr)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "pack bed: null pointer");
  const cuking_status st = cuking_check_block(sm, words_per_sample);
  if (st != CUKING_OK) return st;
  if (site_begin % 64 != 0)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "pack bed: site_begin (%u) must be a multiple of 64", site_begin);
  if (site_begin > site_end || site_end > num_sites)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "pack bed: sites [%u, %u) are not a range inside the %u sites", site_begin,
                       site_end, num_sites);
  if (site_end % 64 != 0 && site_end != num_sites)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "pack bed: site_end (%u) must be a multiple of 64 or the number of sites "
                       "(%u)", site_end, num_sites);
  if (cuking_words_per_sample(num_sites) != words_per_sample)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "pack bed: %u sites need %u words per sample, not %u", num_sites,
                       cuking_words_per_sample(num_sites), words_per_sample);
  if (row_bytes == 0 || row_bytes * 4 < std::max(sm->i_end, sm->j_end))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "pack bed: rows of %llu bytes hold %llu samples, the block reaches "
                       "sample %u", (unsigned long long)row_bytes,
                       (unsigned long long)row_bytes * 4, std::max(sm->i_end, sm->j_end));
  return CUKING_OK;
}

extern "C" {

cuking_status cuking_pack_bed_host(const cuking_submatrix *sm, uint32_t words_per_sample,
                                   uint64_t *bit_set, const uint8_t *bed_rows,
                                   uint64_t row_bytes, uint32_t site_begin, uint32_t site_end,
                                   uint32_t num_sites) {
  const cuking_status st = cuking_check_bed_args(sm, words_per_sample, bit_set, bed_rows,
                                                 row_bytes, site_begin, site_end, num_sites);
  if (st != CUKING_OK) return st;
  if (site_begin == site_end) return CUKING_OK;
  const uint32_t plane_words = words_per_sample / 2;
  const uint64_t word_begin = site_begin / 64, word_end = ((uint64_t)site_end + 63) / 64;
  // The block's stored samples: rows, then the columns of an off-diagonal block.
  const uint32_t begin[2] = {sm->i_begin, sm->j_begin}, end[2] = {sm->i_end, sm->j_end};
  const uint32_t ranges = sm_is_diag(*sm) ? 1u : 2u;
  for (uint64_t w = word_begin; w < word_end; ++w) {
    for (uint32_t r = 0; r < ranges; ++r) {
      for (uint32_t s = begin[r]; s < end[r]; ++s) {
        uint64_t het = 0, hom = 0;
        for (uint32_t bit = 0; bit < 64; ++bit) {
          const uint64_t site = w * 64 + bit;
          // code 1 = missing: what every site past the chunk's (= the file's) last one holds
          uint32_t v = 1;
          if (site < site_end)
            v = (bed_rows[(site - site_begin) * row_bytes + (s >> 2)] >> (2 * (s & 3))) & 3u;
          const uint64_t b0 = v & 1u, b1 = v >> 1;
          het |= (b0 ^ b1) << bit;
          hom |= (b1 ^ 1u) << bit;
        }
        uint64_t *row = bit_set + (uint64_t)sm_sample_offset(*sm, s) * words_per_sample;
        row[w] = het;
        row[w + plane_words] = hom;
      }
    }
  }
  return CUKING_OK;
}

}  // extern "C"

// ---- site QC: the argument checks, the site rule and the host compaction --------------------
cuking_status cuking_check_counts_args(const char *what, const void *bit_set, uint32_t num_stored,
                                       uint32_t words_per_sample, const void *counts) {
  if (words_per_sample == 0 || (words_per_sample & 1))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "%s: words_per_sample must be a positive even number", what);
  if (num_stored != 0 && (bit_set == nullptr || counts == nullptr))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
  return CUKING_OK;
}

cuking_status cuking_check_compact_args(const void *in, uint32_t num_stored,
                                        uint32_t words_per_sample_in, const uint64_t *keep,
                                        uint32_t num_sites_in, const void *out,
                                        uint32_t words_per_sample_out, uint32_t *num_kept) {
  if (in == nullptr || keep == nullptr || out == nullptr)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "compact sites: null pointer");
  if (words_per_sample_in == 0 || (words_per_sample_in & 1) || words_per_sample_out == 0 ||
      (words_per_sample_out & 1))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "compact sites: words_per_sample must be a positive even number");
  if (cuking_words_per_sample(num_sites_in) != words_per_sample_in)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "compact sites: %u sites need %u words per sample, not %u", num_sites_in,
                       cuking_words_per_sample(num_sites_in), words_per_sample_in);
  const uint32_t plane_in = words_per_sample_in / 2;
  uint64_t kept = 0;
  for (uint32_t w = 0; w < plane_in; ++w) {
    const uint64_t first = (uint64_t)w * 64;  // bits of this word at or beyond num_sites_in
    const uint64_t beyond = first >= num_sites_in        ? ~0ull
                            : num_sites_in - first >= 64 ? 0ull
                                                         : ~0ull << (num_sites_in - first);
    if (keep[w] & beyond)
      return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                         "compact sites: the mask keeps site %llu, the input has %u sites",
                         (unsigned long long)(first + (uint64_t)__builtin_ctzll(keep[w] & beyond)),
                         num_sites_in);
    kept += (uint64_t)__builtin_popcountll(keep[w]);
  }
  if (kept == 0) return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "compact sites: no site passes");
  if (cuking_words_per_sample((uint32_t)kept) != words_per_sample_out)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "compact sites: the %llu kept sites need %u words per sample, not %u",
                       (unsigned long long)kept, cuking_words_per_sample((uint32_t)kept),
                       words_per_sample_out);
  const uintptr_t a = reinterpret_cast<uintptr_t>(in), b = reinterpret_cast<uintptr_t>(out);
  const uint64_t a_bytes = (uint64_t)num_stored * words_per_sample_in * 8;
  const uint64_t b_bytes = (uint64_t)num_stored * words_per_sample_out * 8;
  if (a < b + b_bytes && b < a + a_bytes)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "compact sites: the output overlaps the input (the call works out of "
                       "place)");
  if (num_kept != nullptr) *num_kept = (uint32_t)kept;
  return CUKING_OK;
}

extern "C" {

cuking_status cuking_site_mask_host(const uint32_t *counts, uint32_t num_sites,
                                    uint32_t plane_words, const cuking_site_filter *filter,
                                    const uint64_t *also, uint64_t *keep, uint32_t *num_kept) {
  if (counts == nullptr || filter == nullptr || keep == nullptr)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "site mask: null pointer");
  if (plane_words != cuking_words_per_sample(num_sites) / 2)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "site mask: %u sites have %u plane words, not %u", num_sites,
                       cuking_words_per_sample(num_sites) / 2, plane_words);
  // (written so that NaN fails)
  if (!(filter->min_call_rate >= 0.0f && filter->min_call_rate <= 1.0f))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "site mask: min_call_rate (%g) must be in [0, 1]",
                       (double)filter->min_call_rate);
  if (!(filter->min_maf >= 0.0f && filter->min_maf <= 1.0f))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "site mask: min_maf (%g) must be in [0, 1]",
                       (double)filter->min_maf);
  const double min_call_rate = (double)filter->min_call_rate, min_maf = (double)filter->min_maf;
  uint32_t kept = 0;
  for (uint32_t w = 0; w < plane_words; ++w) {
    uint64_t word = 0;
    for (uint32_t bit = 0; bit < 64; ++bit) {
      const uint64_t s = (uint64_t)w * 64 + bit;
      if (s >= num_sites) break;
      const uint32_t *c = counts + s * 4;
      const uint64_t called = (uint64_t)c[0] + c[1] + c[2], n = called + c[3];
      const uint64_t alt = (uint64_t)c[1] + 2 * (uint64_t)c[2];
      const uint64_t minor = std::min(alt, 2 * called - alt);
      const double need_called = min_call_rate * (double)n;
      const double need_minor = min_maf * (double)(2 * called);
      const bool ok = called > 0 && (double)called >= need_called &&
                      (double)minor >= need_minor && minor >= filter->min_mac;
      if (ok) word |= 1ull << bit;
    }
    if (also != nullptr) word &= also[w];
    keep[w] = word;
    kept += (uint32_t)__builtin_popcountll(word);
  }
  if (num_kept != nullptr) *num_kept = kept;
  return CUKING_OK;
}

cuking_status cuking_compact_sites_host(const uint64_t *bit_set_in, uint32_t num_stored,
                                        uint32_t words_per_sample_in, const uint64_t *keep,
                                        uint32_t num_sites_in, uint64_t *bit_set_out,
                                        uint32_t words_per_sample_out) {
  uint32_t kept = 0;
  const cuking_status st =
      cuking_check_compact_args(bit_set_in, num_stored, words_per_sample_in, keep, num_sites_in,
                                bit_set_out, words_per_sample_out, &kept);
  if (st != CUKING_OK) return st;
  const uint32_t plane_in = words_per_sample_in / 2, plane_out = words_per_sample_out / 2;
  for (uint32_t s = 0; s < num_stored; ++s) {
    const uint64_t *in = bit_set_in + (uint64_t)s * words_per_sample_in;
    uint64_t *out = bit_set_out + (uint64_t)s * words_per_sample_out;
    // all missing, then one kept site after the other
    for (uint32_t w = 0; w < words_per_sample_out; ++w) out[w] = ~0ull;
    uint64_t k = 0;
    for (uint64_t site = 0; site < num_sites_in; ++site) {
      if (!((keep[site >> 6] >> (site & 63)) & 1)) continue;
      const uint64_t het = (in[site >> 6] >> (site & 63)) & 1;
      const uint64_t hom = (in[plane_in + (site >> 6)] >> (site & 63)) & 1;
      if (!het) out[k >> 6] &= ~(1ull << (k & 63));
      if (!hom) out[plane_out + (k >> 6)] &= ~(1ull << (k & 63));
      ++k;
    }
  }
  return CUKING_OK;
}

}  // extern "C"

// ---- LD pruning: the argument checks, the host transpose and the host edge list -------------
cuking_status cuking_check_transpose_args(const void *bit_set, uint32_t num_stored,
                                          uint32_t words_per_sample, uint32_t num_sites,
                                          const void *site_bits, uint32_t words_per_site_plane) {
  if (bit_set == nullptr || site_bits == nullptr)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "transpose sites: null pointer");
  if (cuking_words_per_sample(num_sites) != words_per_sample)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "transpose sites: %u sites need %u words per sample, not %u", num_sites,
                       cuking_words_per_sample(num_sites), words_per_sample);
  if (num_stored > kLdMaxStored)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "transpose sites: at most 2^24 samples are served, not %u", num_stored);
  if (ld_site_words(num_stored) != words_per_site_plane)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "transpose sites: %u samples need %u words per site plane, not %u",
                       num_stored, ld_site_words(num_stored), words_per_site_plane);
  return CUKING_OK;
}

cuking_status cuking_check_ld_args(const void *site_bits, uint32_t num_stored, uint32_t window,
                                   float r2_threshold, const void *records, uint64_t max_records,
                                   const void *num_records) {
  if (site_bits == nullptr || num_records == nullptr || (records == nullptr && max_records != 0))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "ld edges: null pointer");
  if (num_stored > kLdMaxStored)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "ld edges: at most 2^24 samples are served, not %u (the sums must stay "
                       "below 2^53)", num_stored);
  if (!ld_window_valid(window))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "ld edges: a window of %u variants holds no pair (at least 2)", window);
  if (!ld_threshold_valid(r2_threshold))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "ld edges: r2_threshold (%g) must be in [0, 1]",
                       (double)r2_threshold);
  return CUKING_OK;
}

cuking_status cuking_ld_count_status(uint64_t count, uint64_t max_records) {
  if (count > kLdMaxEdges)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "ld edges: %llu edges, more than the 2^30 the unrelated set accepts: a "
                       "narrower window or a higher threshold", (unsigned long long)count);
  if (count > max_records)
    return cuking_fail(CUKING_ERR_RESOURCE_EXHAUSTED,
                       "ld edges: %llu edges do not fit %llu records: retry with that many",
                       (unsigned long long)count, (unsigned long long)max_records);
  return CUKING_OK;
}

extern "C" {

uint32_t cuking_ld_site_words(uint32_t num_stored) { return ld_site_words(num_stored); }

float cuking_ld_priority(const uint32_t counts[4]) {
  return counts != nullptr ? ld_priority(counts) : __builtin_nanf("");
}

cuking_status cuking_transpose_sites_host(const uint64_t *bit_set, uint32_t num_stored,
                                          uint32_t words_per_sample, uint32_t num_sites,
                                          uint64_t *site_bits, uint32_t words_per_site_plane) {
  const cuking_status st = cuking_check_transpose_args(bit_set, num_stored, words_per_sample,
                                                       num_sites, site_bits, words_per_site_plane);
  if (st != CUKING_OK) return st;
  const uint32_t plane_words = words_per_sample / 2, q_words = words_per_site_plane;
  for (uint64_t site = 0; site < num_sites; ++site) {
    for (uint32_t plane = 0; plane < 2; ++plane) {
      uint64_t *row = site_bits + (site * 2 + plane) * q_words;
      // all missing (the tail stays so), then one sample after the other
      for (uint32_t q = 0; q < q_words; ++q) row[q] = ~0ull;
      for (uint64_t s = 0; s < num_stored; ++s) {
        const uint64_t word = bit_set[s * words_per_sample + plane * plane_words + (site >> 6)];
        if (!((word >> (site & 63)) & 1)) row[s >> 6] &= ~(1ull << (s & 63));
      }
    }
  }
  return CUKING_OK;
}

cuking_status cuking_ld_edges_host(const uint64_t *site_bits, uint32_t num_sites,
                                   uint32_t num_stored, uint32_t window, float r2_threshold,
                                   const int32_t *group, cuking_result *records,
                                   uint64_t max_records, uint64_t *num_records) {
  if (num_records != nullptr) *num_records = 0;
  const cuking_status st = cuking_check_ld_args(site_bits, num_stored, window, r2_threshold,
                                                records, max_records, num_records);
  if (st != CUKING_OK) return st;
  const uint32_t q_words = ld_site_words(num_stored);
  uint64_t count = 0;
  for (uint64_t a = 0; a < num_sites; ++a) {
    for (uint64_t b = a + 1; ld_pair_in_band(a, b, num_sites, window); ++b) {
      if (group != nullptr && group[a] != group[b]) continue;
      const uint64_t *ra = site_bits + a * 2 * q_words, *rb = site_bits + b * 2 * q_words;
      LdCounts c;
      c.clear();
      for (uint32_t q = 0; q < q_words; ++q) {
        uint64_t na, ha, va, nb, hb, vb;
        ld_masks(ra[q], ra[q_words + q], na, ha, va);
        ld_masks(rb[q], rb[q_words + q], nb, hb, vb);
        c.add(na, ha, va, nb, hb, vb);
      }
      const LdMoments m = ld_moments(c);
      if (!ld_is_edge(m, r2_threshold)) continue;
      if (count < max_records)
        records[count] = cuking_result{(uint32_t)a, (uint32_t)b, ld_r2(m), (uint32_t)m.n, 0, 0};
      ++count;
    }
  }
  *num_records = count;
  return cuking_ld_count_status(count, max_records);
}

}  // extern "C"

// ---- genotype matrix products: the argument checks and the host twin ------------------------
cuking_status cuking_check_geno_args(const void *bits, uint32_t num_rows, uint32_t words_per_row,
                                     uint32_t num_cols, const void *table, int table_axis,
                                     const void *b, uint32_t ldb, uint32_t num_rhs,
                                     const void *out, uint32_t ldo) {
  if (words_per_row == 0 || words_per_row % 2 != 0)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "geno matmul: words_per_row (%u) must be positive and even", words_per_row);
  if (num_cols > 64ull * (words_per_row / 2))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "geno matmul: %u columns do not fit %u plane words (%llu bits)", num_cols,
                       words_per_row / 2, 64ull * (words_per_row / 2));
  if (num_rhs == 0 || num_rhs > kGenoRhsMax)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "geno matmul: num_rhs (%u) must be in [1, %u]", num_rhs, kGenoRhsMax);
  if (ldb < num_rhs || ldo < num_rhs)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "geno matmul: pitches ldb (%u) and ldo (%u) must be at least num_rhs (%u)",
                       ldb, ldo, num_rhs);
  if (!geno_axis_valid(table_axis))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "geno matmul: unknown table axis %d (per column %d, per row %d)",
                       table_axis, kGenoTablePerColumn, kGenoTablePerRow);
  if (num_rows == 0) return CUKING_OK;
  if (out == nullptr)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "geno matmul: null out pointer");
  if (num_cols != 0 && (bits == nullptr || table == nullptr || b == nullptr))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "geno matmul: null pointer");
  return CUKING_OK;
}

extern "C" {

cuking_status cuking_geno_matmul_host(const uint64_t *bits, uint32_t num_rows,
                                      uint32_t words_per_row, uint32_t num_cols,
                                      const float *table, int table_axis, const float *b,
                                      uint32_t ldb, uint32_t num_rhs, float *out, uint32_t ldo) {
  const cuking_status st = cuking_check_geno_args(bits, num_rows, words_per_row, num_cols, table,
                                                  table_axis, b, ldb, num_rhs, out, ldo);
  if (st != CUKING_OK) return st;
  const uint32_t plane_words = words_per_row / 2;
  const bool per_row = table_axis == kGenoTablePerRow;
  std::vector<double> acc(num_rhs);
  for (uint64_t r = 0; r < num_rows; ++r) {
    std::fill(acc.begin(), acc.end(), 0.0);
    const uint64_t *row = num_cols != 0 ? bits + r * words_per_row : nullptr;
    for (uint64_t k = 0; k < num_cols; ++k) {
      const uint32_t code = geno_code(row[k >> 6], row[plane_words + (k >> 6)], (uint32_t)(k & 63));
      const double t = (double)table[(per_row ? r : k) * 4 + code];
      const float *bk = b + k * ldb;
      for (uint32_t c = 0; c < num_rhs; ++c) acc[c] += t * (double)bk[c];
    }
    for (uint32_t c = 0; c < num_rhs; ++c) out[r * ldo + c] = (float)acc[c];
  }
  return CUKING_OK;
}

}  // extern "C"

// ---- PC-Relate: the argument checks and the host twin ---------------------------------------
namespace {

// What the matrix and the listed pairs share: the model's shape and the bounds.
cuking_status check_pcrelate_model(uint32_t words_per_sample, uint32_t num_sites, uint32_t ldx,
                                   uint32_t ldbeta, uint32_t d, float lo, float hi) {
  if (d == 0 || d > kPcrelateColumnsMax)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "pcrelate: d (%u) must be in [1, %u]", d,
                       kPcrelateColumnsMax);
  if (ldx < d || ldbeta < d)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "pcrelate: pitches ldx (%u) and ldbeta (%u) must be at least d (%u)", ldx,
                       ldbeta, d);
  if (num_sites > 64ull * (words_per_sample / 2))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "pcrelate: %u sites do not fit %u plane words (%llu bits)", num_sites,
                       words_per_sample / 2, 64ull * (words_per_sample / 2));
  if (!pcrelate_bounds_valid(lo, hi))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "pcrelate: bounds lo = %g, hi = %g are not 0 <= lo < hi <= 1", (double)lo,
                       (double)hi);
  return CUKING_OK;
}

}  // namespace

namespace {

// What the matrix and the records share: the block, the model and the block inside the stored
// samples.
cuking_status check_pcrelate_block(uint32_t num_stored, uint32_t words_per_sample,
                                   uint32_t num_sites, uint32_t ldx, uint32_t ldbeta, uint32_t d,
                                   float lo, float hi, const cuking_submatrix *block) {
  cuking_status st = cuking_check_block(block, words_per_sample);
  if (st != CUKING_OK) return st;
  st = check_pcrelate_model(words_per_sample, num_sites, ldx, ldbeta, d, lo, hi);
  if (st != CUKING_OK) return st;
  if (block->i_end > num_stored || block->j_end > num_stored)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "pcrelate: block rows [%u, %u) x columns [%u, %u) outside the %u stored "
                       "samples", block->i_begin, block->i_end, block->j_begin, block->j_end,
                       num_stored);
  return CUKING_OK;
}

}  // namespace

cuking_status cuking_check_pcrelate_args(const void *bits, uint32_t num_stored,
                                         uint32_t words_per_sample, uint32_t num_sites,
                                         const void *x, uint32_t ldx, const void *beta,
                                         uint32_t ldbeta, uint32_t d, float lo, float hi,
                                         const cuking_submatrix *block, const void *out,
                                         uint64_t ldo) {
  const cuking_status st = check_pcrelate_block(num_stored, words_per_sample, num_sites, ldx,
                                                ldbeta, d, lo, hi, block);
  if (st != CUKING_OK) return st;
  if (ldo < sm_num_cols(*block))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "pcrelate: output pitch %llu below the block's %u columns",
                       (unsigned long long)ldo, sm_num_cols(*block));
  if (sm_num_rows(*block) == 0 || sm_num_cols(*block) == 0) return CUKING_OK;
  if (out == nullptr)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "pcrelate: null out pointer");
  if (num_sites != 0 && (bits == nullptr || x == nullptr || beta == nullptr))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "pcrelate: null pointer");
  return CUKING_OK;
}

cuking_status cuking_check_pcrelate_records_args(const void *bits, uint32_t num_stored,
                                                 uint32_t words_per_sample, uint32_t num_sites,
                                                 const void *x, uint32_t ldx, const void *beta,
                                                 uint32_t ldbeta, uint32_t d, float lo, float hi,
                                                 const cuking_submatrix *block, float min_kin,
                                                 const void *records, uint64_t max_records,
                                                 const void *num_records) {
  const cuking_status st = check_pcrelate_block(num_stored, words_per_sample, num_sites, ldx,
                                                ldbeta, d, lo, hi, block);
  if (st != CUKING_OK) return st;
  if (min_kin != min_kin)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "pcrelate records: min_kin is NaN");
  if (num_records == nullptr)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "pcrelate records: null num_records pointer");
  if (records == nullptr && max_records != 0)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "pcrelate records: null records pointer with max_records = %llu",
                       (unsigned long long)max_records);
  if (sm_num_rows(*block) == 0 || sm_num_cols(*block) == 0 || num_sites == 0) return CUKING_OK;
  if (bits == nullptr || x == nullptr || beta == nullptr)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "pcrelate records: null pointer");
  return CUKING_OK;
}

cuking_status cuking_pcrelate_count_status(uint64_t count, uint64_t max_records) {
  if (count > max_records)
    return cuking_fail(CUKING_ERR_RESOURCE_EXHAUSTED,
                       "pcrelate records: %llu records do not fit %llu: retry with that many",
                       (unsigned long long)count, (unsigned long long)max_records);
  return CUKING_OK;
}

namespace {

// The host twin of both calls: visit(i, j, kin) for the pairs of `block` in ascending (i, j),
// i and j counted from the block's first row and column; with `upper_only` the pairs i < j of
// a diagonal block.  Sums in double, rounded once, divided in float32.
template <class Visit>
void pcrelate_host_scan(const uint64_t *bits, uint32_t words_per_sample, uint32_t num_sites,
                        const float *x, uint32_t ldx, const float *beta, uint32_t ldbeta,
                        uint32_t d, float lo, float hi, const cuking_submatrix &block,
                        bool upper_only, Visit visit) {
  const uint32_t rows = sm_num_rows(block), cols = sm_num_cols(block);
  const uint32_t plane_words = words_per_sample / 2;
  // r and v of the block's samples, [sample][site]: rows first, then columns
  const auto expand = [&](uint32_t begin, uint32_t count, std::vector<float> *r,
                          std::vector<float> *v) {
    r->assign((size_t)count * num_sites, 0.0f);
    v->assign((size_t)count * num_sites, 0.0f);
    for (uint32_t k = 0; k < count; ++k) {
      const uint64_t sample = (uint64_t)begin + k;
      const uint64_t *row = bits + sample * words_per_sample;
      for (uint64_t s = 0; s < num_sites; ++s) {
        const uint32_t code = geno_code(row[s >> 6], row[plane_words + (s >> 6)], (uint32_t)(s & 63));
        const float mu = pcrelate_mu(x + sample * ldx, beta + s * ldbeta, d);
        pcrelate_element(code, mu, lo, hi, &(*r)[(size_t)k * num_sites + s],
                         &(*v)[(size_t)k * num_sites + s]);
      }
    }
  };
  std::vector<float> ri, vi, rj, vj;
  expand(block.i_begin, rows, &ri, &vi);
  const bool diag = sm_is_diag(block);
  if (!diag) expand(block.j_begin, cols, &rj, &vj);
  const std::vector<float> &rc = diag ? ri : rj, &vc = diag ? vi : vj;
  for (uint32_t i = 0; i < rows; ++i)
    for (uint32_t j = (diag && upper_only) ? i + 1 : 0; j < cols; ++j) {
      double num = 0.0, den = 0.0;
      const float *a = ri.data() + (size_t)i * num_sites, *b = rc.data() + (size_t)j * num_sites;
      const float *p = vi.data() + (size_t)i * num_sites, *q = vc.data() + (size_t)j * num_sites;
      for (uint32_t s = 0; s < num_sites; ++s) {
        num += (double)a[s] * (double)b[s];
        den += (double)p[s] * (double)q[s];
      }
      visit(i, j, pcrelate_kin((float)num, (float)den));
    }
}

}  // namespace

extern "C" {

cuking_status cuking_pcrelate_matrix_host(const uint64_t *bits, uint32_t num_stored,
                                          uint32_t words_per_sample, uint32_t num_sites,
                                          const float *x, uint32_t ldx, const float *beta,
                                          uint32_t ldbeta, uint32_t d, float lo, float hi,
                                          const cuking_submatrix *block, float *out,
                                          uint64_t ldo) {
  const cuking_status st = cuking_check_pcrelate_args(bits, num_stored, words_per_sample,
                                                      num_sites, x, ldx, beta, ldbeta, d, lo, hi,
                                                      block, out, ldo);
  if (st != CUKING_OK) return st;
  if (sm_num_rows(*block) == 0 || sm_num_cols(*block) == 0) return CUKING_OK;
  pcrelate_host_scan(bits, words_per_sample, num_sites, x, ldx, beta, ldbeta, d, lo, hi, *block,
                     false, [&](uint32_t i, uint32_t j, float kin) {
                       out[(uint64_t)i * ldo + j] = kin;
                     });
  return CUKING_OK;
}

cuking_status cuking_pcrelate_records_host(const uint64_t *bits, uint32_t num_stored,
                                           uint32_t words_per_sample, uint32_t num_sites,
                                           const float *x, uint32_t ldx, const float *beta,
                                           uint32_t ldbeta, uint32_t d, float lo, float hi,
                                           const cuking_submatrix *block, float min_kin,
                                           cuking_result *records, uint64_t max_records,
                                           uint64_t *num_records) {
  if (num_records != nullptr) *num_records = 0;
  const cuking_status st = cuking_check_pcrelate_records_args(
      bits, num_stored, words_per_sample, num_sites, x, ldx, beta, ldbeta, d, lo, hi, block,
      min_kin, records, max_records, num_records);
  if (st != CUKING_OK) return st;
  // (without a site every kin is NaN: no record)
  if (sm_num_rows(*block) == 0 || sm_num_cols(*block) == 0 || num_sites == 0) return CUKING_OK;
  uint64_t count = 0;
  pcrelate_host_scan(bits, words_per_sample, num_sites, x, ldx, beta, ldbeta, d, lo, hi, *block,
                     true, [&](uint32_t i, uint32_t j, float kin) {
                       if (!pcrelate_is_record(kin, min_kin)) return;
                       if (count < max_records)
                         records[count] = cuking_result{block->i_begin + i, block->j_begin + j,
                                                        kin, 0, 0, 0};
                       ++count;
                     });
  *num_records = count;
  return cuking_pcrelate_count_status(count, max_records);
}

uint64_t cuking_pcrelate_triangle_tiles(uint64_t side) {
  return side <= kPcrelateTriangleSideMax ? pcrelate_triangle_tiles(side) : 0;
}

uint64_t cuking_pcrelate_triangle_index(uint64_t side, uint32_t tile_i, uint32_t tile_j) {
  if (side > kPcrelateTriangleSideMax || tile_j >= side || tile_i > tile_j) return UINT64_MAX;
  return pcrelate_triangle_index(side, tile_i, tile_j);
}

uint32_t cuking_pcrelate_triangle_tile(uint64_t side, uint64_t index, uint32_t *tile_i,
                                       uint32_t *tile_j) {
  if (tile_i == nullptr || tile_j == nullptr || side > kPcrelateTriangleSideMax ||
      index >= pcrelate_triangle_tiles(side))
    return 0;
  pcrelate_triangle_tile(side, index, tile_i, tile_j);
  return 1;
}

}  // extern "C"

// ---- PC-Relate for listed pairs --------------------------------------------------------------
cuking_status cuking_check_pcrelate_pairs_args(const void *bits, uint32_t words_per_sample,
                                               uint32_t num_sites, const void *x, uint32_t ldx,
                                               const void *beta, uint32_t ldbeta, uint32_t d,
                                               float lo, float hi, const void *pairs,
                                               uint64_t num_pairs, uint32_t pair_stride,
                                               const void *out) {
  if (words_per_sample == 0 || (words_per_sample & 1))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "words_per_sample (%u) must be a positive even number", words_per_sample);
  const cuking_status st = check_pcrelate_model(words_per_sample, num_sites, ldx, ldbeta, d, lo, hi);
  if (st != CUKING_OK) return st;
  if (!pcrelate_pair_stride_valid(pair_stride))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "pcrelate pairs: pair_stride (%u bytes) must be at least 8 and a multiple "
                       "of 4", pair_stride);
  if (num_pairs == 0) return CUKING_OK;
  if (out == nullptr)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "pcrelate pairs: null out pointer");
  if (pairs == nullptr)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "pcrelate pairs: null pairs pointer");
  if (num_sites != 0 && (bits == nullptr || x == nullptr || beta == nullptr))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "pcrelate pairs: null pointer");
  return CUKING_OK;
}

extern "C" {

cuking_status cuking_pcrelate_pairs_host(const uint64_t *bits, uint32_t num_stored,
                                         uint32_t words_per_sample, uint32_t num_sites,
                                         const float *x, uint32_t ldx, const float *beta,
                                         uint32_t ldbeta, uint32_t d, float lo, float hi,
                                         const float *f, const void *pairs, uint64_t num_pairs,
                                         uint32_t pair_stride, cuking_pcrelate_pair *out) {
  const cuking_status st = cuking_check_pcrelate_pairs_args(bits, words_per_sample, num_sites, x,
                                                            ldx, beta, ldbeta, d, lo, hi, pairs,
                                                            num_pairs, pair_stride, out);
  if (st != CUKING_OK) return st;
  const uint32_t plane_words = words_per_sample / 2;
  for (uint64_t p = 0; p < num_pairs; ++p) {
    uint32_t in[2];
    memcpy(in, static_cast<const unsigned char *>(pairs) + p * pair_stride, sizeof(in));
    PcrelatePairSums sum;
    if (in[0] < num_stored && in[1] < num_stored && num_sites != 0) {
      // (the smaller index leads the chains, as on the device)
      const uint64_t si = in[0] < in[1] ? in[0] : in[1], sj = in[0] < in[1] ? in[1] : in[0];
      const uint64_t *row_i = bits + si * words_per_sample, *row_j = bits + sj * words_per_sample;
      const float one_plus_f_i = f != nullptr ? 1.0f + f[si] : 1.0f;
      const float one_plus_f_j = f != nullptr ? 1.0f + f[sj] : 1.0f;
      for (uint64_t s = 0; s < num_sites; ++s) {
        const uint32_t bit = (uint32_t)(s & 63);
        const float *b = beta + s * ldbeta;
        pcrelate_pair_site(&sum, geno_code(row_i[s >> 6], row_i[plane_words + (s >> 6)], bit),
                           pcrelate_mu(x + si * ldx, b, d), one_plus_f_i,
                           geno_code(row_j[s >> 6], row_j[plane_words + (s >> 6)], bit),
                           pcrelate_mu(x + sj * ldx, b, d), one_plus_f_j, lo, hi);
      }
    }
    cuking_pcrelate_pair row;
    row.sample_i = in[0];
    row.sample_j = in[1];
    pcrelate_pair_result(sum, &row.kin, &row.k0, &row.k1, &row.k2);
    row.ibs0 = sum.ibs0;
    row.sites = sum.sites;
    out[p] = row;
  }
  return CUKING_OK;
}

}  // extern "C"

// ---- IBD segments for listed pairs -------------------------------------------------------------
cuking_status cuking_check_ibd_args(const void *bits, uint32_t words_per_sample,
                                    uint32_t num_sites, uint32_t min_sites, const void *pairs,
                                    uint64_t num_pairs, uint32_t pair_stride, const void *out,
                                    const void *segments, uint64_t max_segments,
                                    const void *num_segments) {
  if (words_per_sample == 0 || (words_per_sample & 1))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "words_per_sample (%u) must be a positive even number", words_per_sample);
  if (num_sites > 64ull * (words_per_sample / 2))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "ibd pairs: %u sites do not fit %u plane words (%llu bits)", num_sites,
                       words_per_sample / 2, 64ull * (words_per_sample / 2));
  if (min_sites < kIbdMinSites)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "ibd pairs: min_sites (%u) must be at least %u: a run of %u or more sites "
                       "always closes in a later 64-site word than it starts in, so the scan "
                       "never enumerates the runs inside one word", min_sites, kIbdMinSites,
                       kIbdMinSites);
  if (!pcrelate_pair_stride_valid(pair_stride))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "ibd pairs: pair_stride (%u bytes) must be at least 8 and a multiple of 4",
                       pair_stride);
  if (num_segments == nullptr && (segments != nullptr || max_segments != 0))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "ibd pairs: a segment buffer needs a num_segments pointer");
  if (num_segments != nullptr && num_pairs > (1ull << 32))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "ibd pairs: a segment list names its pair in 32 bits, %llu pairs are too "
                       "many", (unsigned long long)num_pairs);
  if (num_pairs == 0) return CUKING_OK;
  if (out == nullptr)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "ibd pairs: null out pointer");
  if (pairs == nullptr)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "ibd pairs: null pairs pointer");
  if (max_segments != 0 && segments == nullptr)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "ibd pairs: null segments pointer");
  if (num_sites != 0 && bits == nullptr)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "ibd pairs: null bits pointer");
  return CUKING_OK;
}

cuking_status cuking_check_ibd_positions(const int32_t *group, const uint32_t *pos,
                                         uint32_t num_sites) {
  if (pos == nullptr) return CUKING_OK;
  for (uint64_t s = 1; s < num_sites; ++s)
    if (!ibd_group_start(group, num_sites, s) && pos[s] < pos[s - 1])
      return cuking_fail(CUKING_ERR_FAILED_PRECONDITION,
                         "ibd pairs: pos must not decrease inside a group, but pos[%llu] = %u "
                         "follows pos[%llu] = %u", (unsigned long long)s, pos[s],
                         (unsigned long long)(s - 1), pos[s - 1]);
  return CUKING_OK;
}

cuking_status cuking_ibd_count_status(uint64_t count, uint64_t max_segments) {
  if (count > max_segments)
    return cuking_fail(CUKING_ERR_RESOURCE_EXHAUSTED,
                       "ibd pairs: %llu segments do not fit %llu: retry with that many",
                       (unsigned long long)count, (unsigned long long)max_segments);
  return CUKING_OK;
}

cuking_status cuking_check_ibd_bridge(uint32_t bridge_sites) {
  if (bridge_sites != 0 && bridge_sites < kIbdMinSites)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "ibd pairs: bridge_sites (%u) must be 0 or at least %u: a run of %u or more "
                       "sites always closes in a later 64-site word than it starts in, so a "
                       "bridged break is the only break of its word", bridge_sites, kIbdMinSites,
                       kIbdMinSites);
  return CUKING_OK;
}

namespace {

// The group-start bitmask of a call, as the device builds it.
std::vector<uint64_t> ibd_group_bits(const int32_t *group, uint32_t num_sites) {
  std::vector<uint64_t> group_bits(ibd_scan_words(num_sites), 0);
  for (uint64_t s = 0; s <= num_sites; ++s)
    if (ibd_group_start(group, num_sites, s)) group_bits[s >> 6] |= 1ull << (s & 63);
  return group_bits;
}

// The words of ONE subject (a pair: two kinds; a sample against itself: one), one at a time, the
// walk every host twin shares.  in_run(w, valid, in) gives the kKinds `in` masks of word w, valid
// & ~break (valid != 0 implies w < plane_words: only then may it load).  The runs that cross a
// word edge arrive by (word of b + 1, kind) and go through the kind's chain: bridge_sites == 0
// links nothing and tests every run where it closes; otherwise a chain is tested when the next
// run is not linked to it, the last one after the walk.  sums[k] takes the segments of kind
// k + 1, and on_segment(k, a, b, links) is called for each.
template <uint32_t kKinds, class InRun, class OnSegment>
void ibd_walk_sums(uint32_t num_sites, const std::vector<uint64_t> &group_bits,
                   const uint32_t *pos, uint32_t min_sites, uint32_t min_length,
                   uint32_t bridge_sites, IbdKindSums *sums, InRun in_run, OnSegment on_segment) {
  // THE segment test of a chain [a, b] with `links` bridged breaks
  auto test = [&](uint32_t k, uint32_t a, uint32_t b, uint32_t links) {
    const uint32_t pos_a = pos != nullptr ? pos[a] : a, pos_b = pos != nullptr ? pos[b] : b;
    if (!ibd_is_segment(a, b, pos_a, pos_b, min_sites, min_length)) return;
    sums[k].add(pos_b - pos_a);
    sums[k].bridged += links;
    on_segment(k, a, b, links);
  };
  IbdWalk walk[kKinds];
  IbdChain chain[kKinds];
  uint32_t a, b, first, end, links;
  for (uint64_t w = 0; w < group_bits.size(); ++w) {
    uint64_t in[kKinds];
    in_run(w, ibd_valid_mask(num_sites, w), in);
    for (uint32_t k = 0; k < kKinds; ++k)
      if (walk[k].step(in[k], group_bits[w], w, &a, &b) &&
          chain[k].step(a, b, bridge_sites, group_bits.data(), &first, &end, &links))
        test(k, first, end, links);
  }
  for (uint32_t k = 0; k < kKinds; ++k)
    if (chain[k].flush(&first, &end, &links)) test(k, first, end, links);
}

// Both kinds of ONE pair (i, j): the break masks are ibd_opp and ibd_diff of its four planes.
template <class OnSegment>
void ibd_pair_sums(const uint64_t *bits, uint32_t words_per_sample, uint32_t num_sites,
                   const std::vector<uint64_t> &group_bits, const uint32_t *pos,
                   uint32_t min_sites, uint32_t min_length, uint32_t bridge_sites, uint64_t i,
                   uint64_t j, IbdKindSums sums[2], OnSegment on_segment) {
  const uint64_t *row_i = bits + i * words_per_sample, *row_j = bits + j * words_per_sample;
  const uint32_t plane_words = words_per_sample / 2;
  ibd_walk_sums<2>(
      num_sites, group_bits, pos, min_sites, min_length, bridge_sites, sums,
      [&](uint64_t w, uint64_t valid, uint64_t in[2]) {
        uint64_t het_i = 0, hom_i = 0, het_j = 0, hom_j = 0;
        if (valid != 0) {
          het_i = row_i[w];
          hom_i = row_i[plane_words + w];
          het_j = row_j[w];
          hom_j = row_j[plane_words + w];
        }
        in[0] = valid & ~ibd_opp(het_i, hom_i, het_j, hom_j);
        in[1] = valid & ~ibd_diff(het_i, hom_i, het_j, hom_j);
      },
      on_segment);
}

// Rows, bridged counts and the segment list of both host calls.
cuking_status ibd_pairs_host(const uint64_t *bits, uint32_t num_stored, uint32_t words_per_sample,
                             uint32_t num_sites, const int32_t *group, const uint32_t *pos,
                             uint32_t min_sites, uint32_t min_length, uint32_t bridge_sites,
                             const void *pairs, uint64_t num_pairs, uint32_t pair_stride,
                             cuking_ibd_pair *out, uint32_t *bridged,
                             cuking_ibd_segment *segments, uint64_t max_segments,
                             uint64_t *num_segments) {
  if (num_segments != nullptr) *num_segments = 0;
  cuking_status st = cuking_check_ibd_args(bits, words_per_sample, num_sites, min_sites, pairs,
                                           num_pairs, pair_stride, out, segments, max_segments,
                                           num_segments);
  if (st != CUKING_OK) return st;
  st = cuking_check_ibd_bridge(bridge_sites);
  if (st != CUKING_OK) return st;
  if (num_pairs == 0) return CUKING_OK;
  st = cuking_check_ibd_positions(group, pos, num_sites);
  if (st != CUKING_OK) return st;
  const std::vector<uint64_t> group_bits = ibd_group_bits(group, num_sites);
  uint64_t count = 0;
  for (uint64_t p = 0; p < num_pairs; ++p) {
    uint32_t in[2];
    memcpy(in, static_cast<const unsigned char *>(pairs) + p * pair_stride, sizeof(in));
    IbdKindSums sums[2];
    if (in[0] < num_stored && in[1] < num_stored)
      ibd_pair_sums(bits, words_per_sample, num_sites, group_bits, pos, min_sites, min_length,
                    bridge_sites, in[0], in[1], sums,
                    [&](uint32_t k, uint32_t a, uint32_t b, uint32_t) {
                      if (num_segments == nullptr) return;
                      if (count < max_segments)
                        segments[count] = cuking_ibd_segment{(uint32_t)p, k + 1, a, b};
                      ++count;
                    });
    cuking_ibd_pair row;
    row.sample_i = in[0];
    row.sample_j = in[1];
    row.segments1 = sums[0].segments;
    row.segments2 = sums[1].segments;
    row.length1 = sums[0].length;
    row.length2 = sums[1].length;
    row.longest1 = sums[0].longest;
    row.longest2 = sums[1].longest;
    out[p] = row;
    if (bridged != nullptr) {
      bridged[2 * p] = sums[0].bridged;
      bridged[2 * p + 1] = sums[1].bridged;
    }
  }
  if (num_segments == nullptr) return CUKING_OK;
  *num_segments = count;
  return cuking_ibd_count_status(count, max_segments);
}

}  // namespace

// ---- runs of homozygosity ----------------------------------------------------------------------
cuking_status cuking_check_roh_args(const void *bits, uint32_t words_per_sample,
                                    uint32_t num_sites, uint32_t min_sites, uint32_t bridge_sites,
                                    uint64_t num_samples, const void *out, const void *segments,
                                    uint64_t max_segments, const void *num_segments) {
  // The checks of the pair calls, in their order and with their messages.  The list of samples
  // may be null and has no stride: `out` stands in for it (a null `out` is refused first).
  const cuking_status st =
      cuking_check_ibd_args(bits, words_per_sample, num_sites, min_sites, out, num_samples,
                            2 * sizeof(uint32_t), out, segments, max_segments, num_segments);
  return st != CUKING_OK ? st : cuking_check_ibd_bridge(bridge_sites);
}

extern "C" {

// The walk of the pair calls for one sample against itself: one kind, whose break mask is
// roh_break of the sample's two planes.
cuking_status cuking_roh_samples_host(const uint64_t *bits, uint32_t num_stored,
                                      uint32_t words_per_sample, uint32_t num_sites,
                                      const int32_t *group, const uint32_t *pos,
                                      uint32_t min_sites, uint32_t min_length,
                                      uint32_t bridge_sites, const uint32_t *samples,
                                      uint64_t num_samples, cuking_roh_sample *out,
                                      cuking_ibd_segment *segments, uint64_t max_segments,
                                      uint64_t *num_segments) {
  if (num_segments != nullptr) *num_segments = 0;
  cuking_status st = cuking_check_roh_args(bits, words_per_sample, num_sites, min_sites,
                                           bridge_sites, num_samples, out, segments,
                                           max_segments, num_segments);
  if (st != CUKING_OK) return st;
  if (num_samples == 0) return CUKING_OK;
  st = cuking_check_ibd_positions(group, pos, num_sites);
  if (st != CUKING_OK) return st;
  const std::vector<uint64_t> group_bits = ibd_group_bits(group, num_sites);
  const uint32_t plane_words = words_per_sample / 2;
  uint64_t count = 0;
  for (uint64_t r = 0; r < num_samples; ++r) {
    const uint64_t sample = samples != nullptr ? samples[r] : r;
    IbdKindSums sums;
    if (sample < num_stored) {
      const uint64_t *row = bits + sample * words_per_sample;
      ibd_walk_sums<1>(
          num_sites, group_bits, pos, min_sites, min_length, bridge_sites, &sums,
          [&](uint64_t w, uint64_t valid, uint64_t in[1]) {
            in[0] = valid != 0 ? valid & ~roh_break(row[w], row[plane_words + w]) : 0;
          },
          [&](uint32_t, uint32_t a, uint32_t b, uint32_t) {
            if (num_segments == nullptr) return;
            if (count < max_segments)
              segments[count] = cuking_ibd_segment{(uint32_t)r, CUKING_ROH_KIND, a, b};
            ++count;
          });
    }
    cuking_roh_sample row_out;
    row_out.length = sums.length;
    row_out.sample = (uint32_t)sample;
    row_out.segments = sums.segments;
    row_out.longest = sums.longest;
    row_out.bridged = sums.bridged;
    out[r] = row_out;
  }
  if (num_segments == nullptr) return CUKING_OK;
  *num_segments = count;
  return cuking_ibd_count_status(count, max_segments);
}

}  // extern "C"

// ---- IBD scan of a block -----------------------------------------------------------------------
cuking_status cuking_check_ibd_scan_args(const void *bits, uint32_t num_stored,
                                         uint32_t words_per_sample, uint32_t num_sites,
                                         uint32_t min_sites, const cuking_submatrix *block,
                                         const void *records, uint64_t max_records,
                                         const void *num_records) {
  cuking_status st = cuking_check_block(block, words_per_sample);
  if (st != CUKING_OK) return st;
  // (words_per_sample, num_sites and min_sites: the checks of the listed call, with no list)
  st = cuking_check_ibd_args(bits, words_per_sample, num_sites, min_sites, nullptr, 0,
                             2 * sizeof(uint32_t), nullptr, nullptr, 0, nullptr);
  if (st != CUKING_OK) return st;
  if (block->i_end > num_stored || block->j_end > num_stored)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "ibd scan: block rows [%u, %u) x columns [%u, %u) outside the %u stored "
                       "samples", block->i_begin, block->i_end, block->j_begin, block->j_end,
                       num_stored);
  if (num_records == nullptr)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "ibd scan: null num_records pointer");
  if (records == nullptr && max_records != 0)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "ibd scan: null records pointer with max_records = %llu",
                       (unsigned long long)max_records);
  if (sm_num_rows(*block) == 0 || sm_num_cols(*block) == 0 || num_sites == 0) return CUKING_OK;
  if (bits == nullptr)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "ibd scan: null bits pointer");
  return CUKING_OK;
}

cuking_status cuking_ibd_scan_count_status(uint64_t count, uint64_t max_records) {
  if (count > max_records)
    return cuking_fail(CUKING_ERR_RESOURCE_EXHAUSTED,
                       "ibd scan: %llu records do not fit %llu: retry with that many",
                       (unsigned long long)count, (unsigned long long)max_records);
  return CUKING_OK;
}

extern "C" {

// The pairs of the block in ascending (i, j), each through the walk of the listed call's twin.
cuking_status cuking_ibd_scan_host(const uint64_t *bits, uint32_t num_stored,
                                   uint32_t words_per_sample, uint32_t num_sites,
                                   const int32_t *group, const uint32_t *pos, uint32_t min_sites,
                                   uint32_t min_length, const cuking_submatrix *block,
                                   uint64_t min_total, cuking_ibd_pair *records,
                                   uint64_t max_records, uint64_t *num_records) {
  if (num_records != nullptr) *num_records = 0;
  cuking_status st = cuking_check_ibd_scan_args(bits, num_stored, words_per_sample, num_sites,
                                                min_sites, block, records, max_records,
                                                num_records);
  if (st != CUKING_OK) return st;
  // (without a site no run exists: no record)
  if (sm_num_rows(*block) == 0 || sm_num_cols(*block) == 0 || num_sites == 0) return CUKING_OK;
  st = cuking_check_ibd_positions(group, pos, num_sites);
  if (st != CUKING_OK) return st;
  const std::vector<uint64_t> group_bits = ibd_group_bits(group, num_sites);
  const bool diag = sm_is_diag(*block);
  uint64_t count = 0;
  for (uint64_t i = block->i_begin; i < block->i_end; ++i)
    for (uint64_t j = diag ? i + 1 : block->j_begin; j < block->j_end; ++j) {
      IbdKindSums sums[2];
      ibd_pair_sums(bits, words_per_sample, num_sites, group_bits, pos, min_sites, min_length, 0,
                    i, j, sums, [](uint32_t, uint32_t, uint32_t, uint32_t) {});
      if (sums[0].segments < 1 || sums[0].length < min_total) continue;
      if (count < max_records)
        records[count] = cuking_ibd_pair{(uint32_t)i,     (uint32_t)j,    sums[0].segments,
                                         sums[1].segments, sums[0].length, sums[1].length,
                                         sums[0].longest,  sums[1].longest};
      ++count;
    }
  *num_records = count;
  return cuking_ibd_scan_count_status(count, max_records);
}

}  // extern "C"

// ---- Mendelian errors --------------------------------------------------------------------------
cuking_status cuking_check_mendel_args(const void *bits, uint32_t words_per_sample,
                                       uint32_t num_sites, const void *trios, uint64_t num_trios,
                                       const void *out) {
  if (words_per_sample == 0 || (words_per_sample & 1))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "words_per_sample (%u) must be a positive even number", words_per_sample);
  if (num_sites > 64ull * (words_per_sample / 2))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "mendel trios: %u sites do not fit %u plane words (%llu bits)", num_sites,
                       words_per_sample / 2, 64ull * (words_per_sample / 2));
  if (num_trios == 0) return CUKING_OK;
  if (out == nullptr)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "mendel trios: null out pointer");
  if (trios == nullptr)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "mendel trios: null trios pointer");
  if (num_sites != 0 && bits == nullptr)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "mendel trios: null bits pointer");
  return CUKING_OK;
}

cuking_status cuking_check_mendel_site_args(const void *error_bits, uint64_t num_trios,
                                            uint32_t plane_words, const void *counts) {
  if (plane_words == 0)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "mendel site counts: the mask must have at least one word per trio");
  if (num_trios >= (1ull << 32))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "mendel site counts: a count has 32 bits, %llu trios are too many for one "
                       "call", (unsigned long long)num_trios);
  if (num_trios != 0 && (error_bits == nullptr || counts == nullptr))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "mendel site counts: null pointer");
  return CUKING_OK;
}

extern "C" {

// The words of a trio, one at a time, with the functions of king_mendel.h.
cuking_status cuking_mendel_trios_host(const uint64_t *bits, uint32_t num_stored,
                                       uint32_t words_per_sample, uint32_t num_sites,
                                       const uint32_t *trios, uint64_t num_trios,
                                       cuking_mendel_trio *out, uint64_t *error_bits) {
  const cuking_status st =
      cuking_check_mendel_args(bits, words_per_sample, num_sites, trios, num_trios, out);
  if (st != CUKING_OK) return st;
  const uint32_t plane_words = words_per_sample / 2;
  for (uint64_t t = 0; t < num_trios; ++t) {
    const uint32_t who[3] = {trios[3 * t], trios[3 * t + 1], trios[3 * t + 2]};
    cuking_mendel_trio row = {};
    row.child = who[0];
    row.father = who[1];
    row.mother = who[2];
    for (uint32_t w = 0; w < plane_words; ++w) {
      const uint64_t valid = ibd_valid_mask(num_sites, w);
      MendelWord x[3];  // child, father, mother; an absent sample stays missing everywhere
      for (int k = 0; k < 3; ++k)
        if (valid != 0 && who[0] < num_stored && who[k] < num_stored) {
          const uint64_t *r = bits + (uint64_t)who[k] * words_per_sample;
          x[k] = mendel_word(r[w], r[plane_words + w], valid);
        }
      uint64_t code[kMendelCodes], any = 0;
      mendel_code_masks(x[1], x[2], x[0], code);
      for (uint32_t k = 0; k < kMendelCodes; ++k) {
        row.errors[k] += (uint32_t)__builtin_popcountll(code[k]);
        any |= code[k];
      }
      row.called += (uint32_t)__builtin_popcountll(
          mendel_called(x[1], who[1] != kMendelNoParent, x[2], who[2] != kMendelNoParent, x[0]));
      if (error_bits != nullptr) error_bits[t * plane_words + w] = any;
    }
    out[t] = row;
  }
  return CUKING_OK;
}

cuking_status cuking_mendel_site_counts_host(const uint64_t *error_bits, uint64_t num_trios,
                                             uint32_t plane_words, uint32_t *counts) {
  const cuking_status st =
      cuking_check_mendel_site_args(error_bits, num_trios, plane_words, counts);
  if (st != CUKING_OK) return st;
  for (uint64_t t = 0; t < num_trios; ++t)
    for (uint32_t w = 0; w < plane_words; ++w)
      for (uint64_t x = error_bits[t * plane_words + w]; x != 0; x &= x - 1)
        ++counts[(uint64_t)w * 64 + (uint32_t)__builtin_ctzll(x)];
  return CUKING_OK;
}

}  // extern "C"

// ---- Hardy-Weinberg test -------------------------------------------------------------------------
cuking_status cuking_check_hwe_args(const void *counts, uint32_t num_sites, uint32_t flags,
                                    const void *p) {
  if (flags & ~CUKING_HWE_MIDP)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "hwe sites: unknown flags 0x%x", flags);
  if (num_sites != 0 && (counts == nullptr || p == nullptr))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "hwe sites: null pointer");
  return CUKING_OK;
}

extern "C" {

// The sites one at a time, with the function of king_hwe.h.
cuking_status cuking_hwe_sites_host(const uint32_t *counts, uint32_t num_sites, uint32_t flags,
                                    double *p) {
  const cuking_status st = cuking_check_hwe_args(counts, num_sites, flags, p);
  if (st != CUKING_OK) return st;
  for (uint32_t s = 0; s < num_sites; ++s) {
    const uint32_t *c = counts + (uint64_t)s * 4;
    p[s] = hwe_exact_p(c[0], c[1], c[2], (flags & CUKING_HWE_MIDP) != 0);
  }
  return CUKING_OK;
}

}  // extern "C"

// ---- PI_HAT (PLINK --genome) -----------------------------------------------------------------
cuking_status cuking_check_pihat_args(const cuking_pihat_model *model, uint32_t flags) {
  if (flags & ~CUKING_PIHAT_UNBOUNDED)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "pi_hat: unknown flags 0x%x", flags);
  if (model == nullptr)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "pi_hat: null model pointer");
  return CUKING_OK;
}

extern "C" {

// The sites one at a time, with the functions of king_pihat.h.
cuking_status cuking_pihat_model_host(const uint32_t *counts, uint32_t num_sites,
                                      cuking_pihat_model *model) {
  if (model == nullptr)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "pi_hat model: null model pointer");
  if (num_sites != 0 && counts == nullptr)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "pi_hat model: null counts pointer");
  uint32_t bad = 0;
  cuking_pihat_model m = {};
  if (!pihat_model_of_counts(counts, num_sites, &m, &bad))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "pi_hat model: site %u counts more than 2^24 people", bad);
  *model = m;
  return CUKING_OK;
}

cuking_status cuking_pihat_records_host(const cuking_result *records, uint64_t num_records,
                                        const cuking_pihat_model *model, uint32_t flags,
                                        double *out) {
  const cuking_status st = cuking_check_pihat_args(model, flags);
  if (st != CUKING_OK) return st;
  if (num_records != 0 && (records == nullptr || out == nullptr))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "pi_hat records: null pointer");
  for (uint64_t k = 0; k < num_records; ++k)
    pihat_z_of_counts(model->e00, model->e01, model->e02, model->e11, model->e12,
                      records[k].ibs0, records[k].ibs1, records[k].ibs2,
                      (flags & CUKING_PIHAT_UNBOUNDED) == 0, out + 4 * k);
  return CUKING_OK;
}

// The pairs of the block in ascending (i, j), each counted with plain popcounts over the words
// of the two samples (cuking.cu:216-240 for the sums; ibs0/1/2 as a KING record carries them).
cuking_status cuking_compute_pihat_host(const cuking_submatrix *sm, uint32_t words_per_sample,
                                        const uint64_t *bit_sets,
                                        const cuking_pihat_model *model, float min_pi_hat,
                                        uint32_t flags, uint32_t max_results,
                                        cuking_result *results, uint32_t *num_results) {
  if (num_results != nullptr) *num_results = 0;
  cuking_status st = cuking_check_block(sm, words_per_sample);
  if (st != CUKING_OK) return st;
  st = cuking_check_pihat_args(model, flags);
  if (st != CUKING_OK) return st;
  if (num_results == nullptr || (max_results != 0 && results == nullptr))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "pi_hat: null result pointer");
  if (sm_num_rows(*sm) == 0 || sm_num_cols(*sm) == 0) return CUKING_OK;
  if (bit_sets == nullptr)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "pi_hat: null bitset pointer");
  const bool diag = sm_is_diag(*sm);
  const uint32_t plane_words = words_per_sample / 2;
  uint64_t count = 0;
  for (uint64_t i = sm->i_begin; i < sm->i_end; ++i) {
    const uint64_t *si = bit_sets + (i - sm->i_begin) * words_per_sample;
    for (uint64_t j = diag ? i + 1 : sm->j_begin; j < sm->j_end; ++j) {
      const uint64_t stored_j = diag ? j - sm->j_begin : sm_num_rows(*sm) + (j - sm->j_begin);
      const uint64_t *sj = bit_sets + stored_j * words_per_sample;
      uint32_t ibs0 = 0, ibs2 = 0, shared = 0;
      for (uint32_t w = 0; w < plane_words; ++w) {
        const uint64_t hi = si[w], ai = si[plane_words + w];
        const uint64_t hj = sj[w], aj = sj[plane_words + w];
        const uint64_t ri = ~hi & ~ai, rj = ~hj & ~aj;
        const uint64_t defined = ~(hi & ai) & ~(hj & aj);
        ibs0 += (uint32_t)__builtin_popcountll(((ri & aj) | (ai & rj)) & defined);
        ibs2 += (uint32_t)__builtin_popcountll(((ri & rj) | (ai & aj) | (hi & hj)) & defined);
        shared += (uint32_t)__builtin_popcountll(defined);
      }
      const uint32_t ibs1 = shared - ibs0 - ibs2;
      const float pi_hat = pihat_of_counts(model->e00, model->e01, model->e02, model->e11,
                                           model->e12, ibs0, ibs1, ibs2, flags);
      if (!(pi_hat > min_pi_hat)) continue;
      if (count < max_results)
        results[count] = cuking_result{(uint32_t)i, (uint32_t)j, pi_hat, ibs0, ibs1, ibs2};
      ++count;
    }
  }
  *num_results = (uint32_t)(count > 0xFFFFFFFFull ? 0xFFFFFFFFull : count);
  if (count > max_results)
    return cuking_fail(CUKING_ERR_RESOURCE_EXHAUSTED,
                       "pi_hat: %llu records do not fit %u: retry with that many",
                       (unsigned long long)count, max_results);
  return CUKING_OK;
}

}  // extern "C"

extern "C" {

cuking_status cuking_ibd_pairs_host(const uint64_t *bits, uint32_t num_stored,
                                    uint32_t words_per_sample, uint32_t num_sites,
                                    const int32_t *group, const uint32_t *pos,
                                    uint32_t min_sites, uint32_t min_length, const void *pairs,
                                    uint64_t num_pairs, uint32_t pair_stride,
                                    cuking_ibd_pair *out, cuking_ibd_segment *segments,
                                    uint64_t max_segments, uint64_t *num_segments) {
  return ibd_pairs_host(bits, num_stored, words_per_sample, num_sites, group, pos, min_sites,
                        min_length, 0, pairs, num_pairs, pair_stride, out, nullptr, segments,
                        max_segments, num_segments);
}

cuking_status cuking_ibd_pairs_bridged_host(const uint64_t *bits, uint32_t num_stored,
                                            uint32_t words_per_sample, uint32_t num_sites,
                                            const int32_t *group, const uint32_t *pos,
                                            uint32_t min_sites, uint32_t min_length,
                                            uint32_t bridge_sites, const void *pairs,
                                            uint64_t num_pairs, uint32_t pair_stride,
                                            cuking_ibd_pair *out, uint32_t *bridged,
                                            cuking_ibd_segment *segments, uint64_t max_segments,
                                            uint64_t *num_segments) {
  return ibd_pairs_host(bits, num_stored, words_per_sample, num_sites, group, pos, min_sites,
                        min_length, bridge_sites, pairs, num_pairs, pair_stride, out, bridged,
                        segments, max_segments, num_segments);
}

}  // extern "C"

extern "C" {

// ---- schedules of a block over the GPUs of a node (host/schedule.h) ----------
void cuking_schedule_tile_partition(uint64_t num_tiles, uint32_t world, uint64_t *out) {
  if (world == 0 || out == nullptr) return;
  const auto parts = cuking_host::TilePartition(num_tiles, world);
  for (uint32_t r = 0; r < world; ++r) {
    out[2 * r] = parts[r].begin;
    out[2 * r + 1] = parts[r].end;
  }
}

cuking_status cuking_schedule_weighted_tile_partition(uint64_t num_tiles, const double *weights,
                                                      uint32_t world, uint64_t *out) {
  if (world == 0 || weights == nullptr || out == nullptr)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null argument");
  std::vector<double> w(weights, weights + world);
  for (double x : w)
    if (!(x > 0) || !std::isfinite(x))
      return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "weights must be positive");
  const auto parts = cuking_host::WeightedTilePartition(num_tiles, w);
  for (uint32_t r = 0; r < world; ++r) {
    out[2 * r] = parts[r].begin;
    out[2 * r + 1] = parts[r].end;
  }
  return CUKING_OK;
}

uint64_t cuking_schedule_calibration_tiles(uint64_t num_tiles, uint32_t world) {
  return cuking_host::CalibrationTiles(num_tiles, world);
}

uint32_t cuking_schedule_chunk_ranges(uint32_t num_samples, uint32_t tile, uint32_t num_chunks,
                                      uint32_t *out) {
  if (tile == 0 || out == nullptr) return 0;
  const auto chunks = cuking_host::ChunkRanges(num_samples, tile, num_chunks);
  for (size_t c = 0; c < chunks.size(); ++c) {
    out[2 * c] = chunks[c].begin;
    out[2 * c + 1] = chunks[c].end;
  }
  return (uint32_t)chunks.size();
}

uint32_t cuking_schedule_staged_steps(uint32_t num_samples, uint32_t tile, uint32_t world,
                                      uint32_t rank, uint32_t num_chunks, uint32_t *out) {
  if (tile == 0 || world == 0 || rank >= world || out == nullptr) return 0;
  const auto steps = cuking_host::StagedSchedule(num_samples, tile, world, rank, num_chunks);
  for (size_t k = 0; k < steps.size(); ++k) {
    uint32_t *o = out + 6 * k;
    o[0] = steps[k].chunk.begin;
    o[1] = steps[k].chunk.end;
    o[2] = steps[k].has_rect ? 1u : 0u;
    o[3] = steps[k].row_begin;
    o[4] = steps[k].row_end;
    o[5] = steps[k].row_step;
  }
  return (uint32_t)steps.size();
}

// ---- kinship summary: the definitions of king_kin_summary.h, as the kernel uses them -----
uint32_t cuking_kin_hist_slots(uint32_t num_bins) { return kin_hist_slots(num_bins); }

uint32_t cuking_kin_bin_slot(const cuking_kin_bins *bins, float kin) {
  if (bins == nullptr || !kin_bins_valid(*bins)) return 0xFFFFFFFFu;
  return kin_bin_slot(bins->lo, kin_bin_scale(*bins), bins->num_bins, kin);
}

uint64_t cuking_kin_best_key(float kin, uint32_t partner) { return kin_best_key(kin, partner); }

uint32_t cuking_kin_best_decode(uint64_t key, float *kin, uint32_t *partner) {
  float k = 0.f;
  uint32_t p = 0;
  if (!kin_best_decode(key, &k, &p)) return 0;
  if (kin != nullptr) *kin = k;
  if (partner != nullptr) *partner = p;
  return 1;
}

// ---- relative counts: the band rule of king_kin_summary.h --------------------------------
uint32_t cuking_rel_band(const float *thresholds, uint32_t num_thresholds, float kin) {
  if (!rel_thresholds_valid(thresholds, num_thresholds)) return kRelNoBand;
  return rel_band(thresholds, num_thresholds, kin);
}

// ---- unrelated set and families: the contract of king_unrelated.h with the plain algorithms --
uint64_t cuking_unrelated_key(float priority, uint32_t sample) { return unrel_key(priority, sample); }

cuking_status cuking_unrelated_set_host(const cuking_result *records, uint64_t num_records,
                                        uint32_t num_samples, float prune_threshold,
                                        const float *priority, uint8_t *keep, uint32_t *family) {
  if (!unrel_threshold_valid(prune_threshold))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "unrelated set: prune_threshold is NaN");
  if (num_records != 0 && records == nullptr)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "unrelated set: null records pointer");
  if (num_samples != 0 && keep == nullptr)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "unrelated set: null keep pointer");
  // The edge set: valid records above the threshold, each pair once.
  std::vector<uint64_t> edges;
  for (uint64_t r = 0; r < num_records; ++r) {
    const cuking_result &rec = records[r];
    if (!unrel_record_valid(rec.sample_i, rec.sample_j, num_samples))
      return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                         "unrelated set: a record does not satisfy sample_i < sample_j < "
                         "num_samples (%u)", num_samples);
    if (unrel_is_edge(rec.kin, prune_threshold))
      edges.push_back(unrel_edge_word(rec.sample_i, rec.sample_j));
  }
  std::sort(edges.begin(), edges.end());
  edges.erase(std::unique(edges.begin(), edges.end()), edges.end());
  // Adjacency (CSR); a sample's row length is its number of distinct partners.
  std::vector<uint64_t> row(num_samples + (size_t)1, 0);
  for (const uint64_t e : edges) {
    ++row[(uint32_t)(e >> 32) + (size_t)1];
    ++row[(uint32_t)e + (size_t)1];
  }
  for (size_t s = 0; s < num_samples; ++s) row[s + 1] += row[s];
  std::vector<uint32_t> adj(2 * edges.size());
  {
    std::vector<uint64_t> fill(row.begin(), row.end() - 1);
    for (const uint64_t e : edges) {
      const uint32_t i = (uint32_t)(e >> 32), j = (uint32_t)e;
      adj[fill[i]++] = j;
      adj[fill[j]++] = i;
    }
  }
  std::vector<uint64_t> key(num_samples);
  for (uint32_t s = 0; s < num_samples; ++s)
    key[s] = unrel_key(priority != nullptr
                           ? priority[s]
                           : unrel_default_priority((uint32_t)(row[s + (size_t)1] - row[s])),
                       s);
  // The sequential greedy in descending key order.
  std::vector<uint32_t> order(num_samples);
  std::iota(order.begin(), order.end(), 0u);
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return key[a] > key[b]; });
  for (uint32_t s = 0; s < num_samples; ++s) keep[s] = kUnrelDropped;
  for (const uint32_t s : order) {
    bool related = false;
    for (uint64_t k = row[s]; k < row[s + (size_t)1] && !related; ++k)
      related = keep[adj[k]] == kUnrelKept;
    if (!related) keep[s] = kUnrelKept;
  }
  if (family == nullptr) return CUKING_OK;
  // Union-find, the lower root wins: a component's root is its lowest index.
  std::vector<uint32_t> parent(num_samples);
  std::iota(parent.begin(), parent.end(), 0u);
  auto find = [&](uint32_t x) {
    while (parent[x] != x) x = parent[x] = parent[parent[x]];
    return x;
  };
  for (const uint64_t e : edges) {
    const uint32_t a = find((uint32_t)(e >> 32)), b = find((uint32_t)e);
    if (a != b) parent[std::max(a, b)] = std::min(a, b);
  }
  for (uint32_t s = 0; s < num_samples; ++s) family[s] = find(s);
  return CUKING_OK;
}

void cuking_sort_results(cuking_result *results, size_t num_results) {
  std::sort(results, results + num_results,
            [](const cuking_result &a, const cuking_result &b) {
              return std::tie(a.sample_i, a.sample_j, a.kin) <
                     std::tie(b.sample_i, b.sample_j, b.kin);
            });
}

}  // extern "C"
