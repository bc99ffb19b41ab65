// LD pruning on the device (include/cuking_amd.h "LD pruning" holds the contract, king_ld.h the
// definitions as code, king_host.cc the specification in executable form; DESIGN.md 4.3c the
// reasons for the shapes): transpose_sites_kernel, ld_edges_kernel.
//
// transpose_sites_kernel -- the sample-major bitset [sample][plane][site word] into site-major
// planes [site][plane][sample word]: the mirror image of pack_bed_kernel.  A workgroup of four
// wavefronts owns kTrWords = 4 input word columns (256 sites) x kTrSamples = 512 samples (8
// output words).
//   load       the 32 contiguous bytes of a sample's four het words, and of its four hom_var
//              words, go to LDS; rows at or beyond num_stored read as all-ones (missing).  LDS
//              rows are 5 words apart: the transposing read walks down a column without bank
//              conflicts.
//   transpose  wavefront c takes word column c.  Per plane and per group of 64 samples, lane l
//              reads the word of sample 64 q + l; the 64 x 64 bit matrix the wavefront then
//              holds is transposed in six exchange steps with lane ^ 32 .. lane ^ 1 (a ballot
//              per site would be 64 steps), which leaves output word q of site 64 w + k in
//              lane k: after the eight groups lane k holds the tile's eight consecutive words
//              of its site's row.
//   store      per plane a lane writes its run of up to 64 contiguous bytes.  Every output word
//              is written once, with a plain store: no atomics, no memset.  Sites >= num_sites
//              of the last input word are dropped, as are words from Q on.
//
// ld_edges_kernel -- the r^2 of every pair of the band 0 < b - a < window, as edges.  A
// workgroup of eight wavefronts owns a pair of tiles of kLdTile = 64 sites: row tile R and one
// of the kLdTile-aligned column tiles R .. R + (kLdTile + window - 2) / kLdTile, the only ones
// the band of R's rows reaches (the band's tiles are enumerated, not the triangle's).  It walks
// the Q sample words in chunks of kLdChunk: the het / hom_var words of its 128 sites (64 on the
// diagonal tile) are loaded once, turned into N, H, V (king_ld.h) and staged in LDS; a thread
// accumulates the nine popcounts of a 2 x 4 register block of pairs (72 uint32 counters, no
// scratch).  A wavefront covers a patch of 16 rows x 32 columns; a patch without a pair inside
// the band (below the diagonal, beyond the window) skips the accumulation and the epilogue.
// The epilogue forms the int64 sums and makes THE double comparison of king_ld.h, counts the
// wavefront's edges with ballots, takes their slots with ONE 64-bit atomic add per wavefront
// that has any, and stores the 24-byte records whose slot is below max_records with plain
// stores: every edge is counted, nothing is written past the buffer.
#include <hip/hip_runtime.h>

#include "king_common.h"
#include "king_device.h"
#include "king_ld.h"

namespace cuking {

namespace {

// ---- transpose ------------------------------------------------------------------------------
constexpr uint32_t kTrThreads = 256;
constexpr uint32_t kTrWords = kTrThreads / 64;   // input word columns of a workgroup: one per wave
constexpr uint32_t kTrGroups = 8;                // groups of 64 samples = output words of a tile
constexpr uint32_t kTrSamples = 64 * kTrGroups;  // 512
constexpr uint32_t kTrLdsStride = kTrWords + 1;  // (odd: conflict-free columns)

struct TransposeArgs {
  const uint64_t *bit_set;
  uint64_t *site_bits;
  uint32_t num_stored, words_per_sample, num_sites;
  uint32_t q_words;     // Q
  uint32_t word_tiles;  // tiles of kTrWords input word columns (over the real sites)
  uint64_t block_base;  // first workgroup of this launch
};

// The 64 x 64 bit matrix "lane l holds row l" transposed across the wavefront: afterwards bit j
// of lane k is what bit k of lane j was.  Six exchange steps (blocks of 32, 16, .. 1): a lane
// keeps the half of its word that stays and takes the other half from lane ^ j.
__device__ inline uint64_t transpose64(uint64_t x, uint32_t lane) {
  constexpr uint64_t kKeep[6] = {0x00000000FFFFFFFFull, 0x0000FFFF0000FFFFull,
                                 0x00FF00FF00FF00FFull, 0x0F0F0F0F0F0F0F0Full,
                                 0x3333333333333333ull, 0x5555555555555555ull};
#pragma unroll
  for (uint32_t step = 0; step < 6; ++step) {
    const uint32_t j = 32u >> step;
    const uint64_t m = kKeep[step];  // the columns without bit j
    const uint32_t y_lo = __shfl_xor((uint32_t)x, (int)j), y_hi = __shfl_xor((uint32_t)(x >> 32), (int)j);
    const uint64_t y = ((uint64_t)y_hi << 32) | y_lo;
    x = (lane & j) ? (x & ~m) | ((y & ~m) >> j) : (x & m) | ((y & m) << j);
  }
  return x;
}

__global__ __launch_bounds__(kTrThreads) void transpose_sites_kernel(const TransposeArgs a) {
  __shared__ uint64_t tile[2 * kTrSamples * kTrLdsStride];
  const uint64_t block = a.block_base + blockIdx.x;
  const uint32_t wt = (uint32_t)(block % a.word_tiles);  // word tiles are the fast index:
  const uint32_t qt = (uint32_t)(block / a.word_tiles);  // neighbours read neighbouring bytes
  const uint32_t plane_words = a.words_per_sample / 2;
  const uint32_t real_words = (uint32_t)(((uint64_t)a.num_sites + 63) / 64);  // <= plane_words
  const uint32_t w0 = wt * kTrWords;
  const uint64_t s0 = (uint64_t)qt * kTrSamples;

  // ---- load: [sample][plane][word] of the tile -> LDS, all loads in flight before a store
  {
    constexpr uint32_t kItems = 2 * kTrSamples * kTrWords / kTrThreads;  // 16 per thread
    uint64_t v[kItems];
#pragma unroll
    for (uint32_t i = 0; i < kItems; ++i) {
      const uint32_t idx = i * kTrThreads + threadIdx.x;
      const uint32_t word = idx % kTrWords, plane = (idx / kTrWords) & 1u;
      const uint64_t s = s0 + idx / (2 * kTrWords);
      const bool in = s < a.num_stored && w0 + word < real_words;
      v[i] = in ? a.bit_set[s * a.words_per_sample + (uint64_t)plane * plane_words + w0 + word]
                : ~0ull;
    }
#pragma unroll
    for (uint32_t i = 0; i < kItems; ++i) {
      const uint32_t idx = i * kTrThreads + threadIdx.x;
      const uint32_t word = idx % kTrWords, plane = (idx / kTrWords) & 1u;
      const uint32_t s = idx / (2 * kTrWords);
      tile[(plane * kTrSamples + s) * kTrLdsStride + word] = v[i];
    }
  }
  __syncthreads();

  // ---- transpose and store: wavefront c owns word column w0 + c
  const uint32_t lane = threadIdx.x & 63u, c = threadIdx.x >> 6;
  if (w0 + c >= real_words) return;  // (whole wavefronts)
  const uint64_t site = ((uint64_t)(w0 + c) << 6) + lane;
  const uint32_t q0 = qt * kTrGroups;
  const uint32_t words = a.q_words - q0 < kTrGroups ? a.q_words - q0 : kTrGroups;  // > 0
#pragma unroll 1
  for (uint32_t plane = 0; plane < 2; ++plane) {
    uint64_t out[kTrGroups];
#pragma unroll
    for (uint32_t g = 0; g < kTrGroups; ++g)
      out[g] = transpose64(tile[(plane * kTrSamples + 64 * g + lane) * kTrLdsStride + c], lane);
    if (site < a.num_sites) {
      uint64_t *dst = a.site_bits + (site * 2 + plane) * a.q_words + q0;
#pragma unroll
      for (uint32_t g = 0; g < kTrGroups; ++g)
        if (g < words) dst[g] = out[g];
    }
  }
}

// ---- edges ----------------------------------------------------------------------------------
constexpr uint32_t kLdTile = 64;                  // sites of a row tile and of a column tile
constexpr uint32_t kLdThreads = 512;              // eight wavefronts
constexpr uint32_t kLdRows = 2, kLdCols = 4;      // a thread's register block of pairs
constexpr uint32_t kLdPatchRows = 8 * kLdRows;    // 16: a wavefront is 8 x 8 threads
constexpr uint32_t kLdPatchCols = 8 * kLdCols;    // 32
constexpr uint32_t kLdChunk = 8;                  // sample words staged at a time
// per site [word of the chunk][N, H, V] and one word of padding: 25 words = 50 dwords apart,
// so that the 8 distinct rows (2 sites apart) and the 8 distinct columns (4 sites apart) a
// wavefront reads with one instruction fall into different banks
constexpr uint32_t kLdSiteStride = 3 * kLdChunk + 1;
static_assert(kLdTile % kLdPatchRows == 0 && kLdTile % kLdPatchCols == 0, "whole patches");
static_assert((kLdTile / kLdPatchRows) * (kLdTile / kLdPatchCols) * 64 == kLdThreads,
              "one wavefront per patch");

struct LdArgs {
  const uint64_t *site_bits;
  const int32_t *group;       // or nullptr
  cuking_result *records;
  unsigned long long *count;
  uint64_t max_records;
  uint32_t num_sites, q_words, window;
  float r2_threshold;
  uint32_t col_tiles;         // column tiles per row tile
  uint64_t block_base;        // first workgroup of this launch
};

__global__ __launch_bounds__(kLdThreads) void ld_edges_kernel(const LdArgs a) {
  __shared__ uint64_t staged[2 * kLdTile * kLdSiteStride];
  const uint64_t block = a.block_base + blockIdx.x;
  const uint64_t row_tile = block / a.col_tiles;
  const uint64_t col_tile = row_tile + block % a.col_tiles;
  const uint64_t row0 = row_tile * kLdTile, col0 = col_tile * kLdTile;
  if (col0 >= a.num_sites) return;  // (the whole workgroup: the last row tiles reach past the end)
  const bool diagonal = col_tile == row_tile;
  const uint32_t sites = diagonal ? kLdTile : 2 * kLdTile;  // staged: rows, then columns

  // this thread's block of pairs: wavefront = patch, 8 x 8 threads inside
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t patch_row = (wave / (kLdTile / kLdPatchCols)) * kLdPatchRows;
  const uint32_t patch_col = (wave % (kLdTile / kLdPatchCols)) * kLdPatchCols;
  const uint32_t r_local = patch_row + (lane >> 3) * kLdRows;
  const uint32_t c_local = patch_col + (lane & 7u) * kLdCols;
  // Does the patch hold a pair of the band?  Its largest b - a must be positive, its smallest
  // below the window (the same for all lanes of the wavefront).
  const int64_t diff_max = (int64_t)(col0 + patch_col + kLdPatchCols - 1) - (int64_t)(row0 + patch_row);
  const int64_t diff_min = (int64_t)(col0 + patch_col) - (int64_t)(row0 + patch_row + kLdPatchRows - 1);
  const bool active = diff_max >= 1 && diff_min < (int64_t)a.window &&
                      row0 + patch_row < a.num_sites && col0 + patch_col < a.num_sites;

  LdCounts acc[kLdRows][kLdCols];
#pragma unroll
  for (uint32_t i = 0; i < kLdRows; ++i)
#pragma unroll
    for (uint32_t j = 0; j < kLdCols; ++j) acc[i][j].clear();

  const uint64_t *rows = staged + (uint64_t)r_local * kLdSiteStride;
  const uint64_t *cols = staged + (uint64_t)((diagonal ? 0u : kLdTile) + c_local) * kLdSiteStride;
  for (uint32_t k0 = 0; k0 < a.q_words; k0 += kLdChunk) {
    __syncthreads();  // (the chunk before has been read)
    // stage: item = (site, word of the chunk); consecutive lanes read consecutive words
    for (uint32_t item = threadIdx.x; item < sites * kLdChunk; item += kLdThreads) {
      const uint32_t s = item / kLdChunk, k = item % kLdChunk;
      const uint64_t site = (s < kLdTile ? row0 : col0 - kLdTile) + s;
      uint64_t het = ~0ull, hom = ~0ull;  // beyond the sites or the words: missing, counts nothing
      if (site < a.num_sites && k0 + k < a.q_words) {
        const uint64_t *p = a.site_bits + site * 2 * a.q_words + k0 + k;
        het = p[0];
        hom = p[a.q_words];
      }
      uint64_t n, h, v;
      ld_masks(het, hom, n, h, v);
      uint64_t *dst = staged + (uint64_t)s * kLdSiteStride + 3 * k;
      dst[0] = n;
      dst[1] = h;
      dst[2] = v;
    }
    __syncthreads();
    if (!active) continue;
#pragma unroll 1
    for (uint32_t k = 0; k < kLdChunk; ++k) {
      uint64_t rn[kLdRows], rh[kLdRows], rv[kLdRows];
#pragma unroll
      for (uint32_t i = 0; i < kLdRows; ++i) {
        const uint64_t *p = rows + i * kLdSiteStride + 3 * k;
        rn[i] = p[0];
        rh[i] = p[1];
        rv[i] = p[2];
      }
#pragma unroll
      for (uint32_t j = 0; j < kLdCols; ++j) {
        const uint64_t *p = cols + j * kLdSiteStride + 3 * k;
        const uint64_t cn = p[0], ch = p[1], cv = p[2];
#pragma unroll
        for (uint32_t i = 0; i < kLdRows; ++i) acc[i][j].add(rn[i], rh[i], rv[i], cn, ch, cv);
      }
    }
  }
  if (!active) return;  // (whole wavefronts)

  // ---- epilogue: the edge rule, one slot allocation per wavefront, plain stores
  uint32_t edge_bits = 0;  // bit i * kLdCols + j: pair (i, j) of this thread is an edge
  uint32_t before[kLdRows * kLdCols];  // edges of the wavefront in front of this pair's
  uint32_t total = 0;
#pragma unroll
  for (uint32_t i = 0; i < kLdRows; ++i) {
#pragma unroll
    for (uint32_t j = 0; j < kLdCols; ++j) {
      const uint64_t sa = row0 + r_local + i, sb = col0 + c_local + j;
      bool edge = ld_pair_in_band(sa, sb, a.num_sites, a.window);
      if (edge && a.group != nullptr) edge = a.group[sa] == a.group[sb];
      if (edge) edge = ld_is_edge(ld_moments(acc[i][j]), a.r2_threshold);
      const uint64_t mask = __ballot(edge);
      before[i * kLdCols + j] = total + (uint32_t)__popcll(mask & ((1ull << lane) - 1));
      total += (uint32_t)__popcll(mask);
      if (edge) edge_bits |= 1u << (i * kLdCols + j);
    }
  }
  if (total == 0) return;  // (the same for every lane)
  unsigned long long base = 0;
  if (lane == 0) base = atomicAdd(a.count, (unsigned long long)total);
  const uint32_t base_lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
  const uint32_t base_hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(base >> 32));
  base = ((unsigned long long)base_hi << 32) | base_lo;
#pragma unroll
  for (uint32_t i = 0; i < kLdRows; ++i) {
#pragma unroll
    for (uint32_t j = 0; j < kLdCols; ++j) {
      if (!(edge_bits & (1u << (i * kLdCols + j)))) continue;
      const uint64_t slot = base + before[i * kLdCols + j];
      if (slot >= a.max_records) continue;
      const LdMoments m = ld_moments(acc[i][j]);
      cuking_result *out = a.records + slot;
      out->sample_i = (uint32_t)(row0 + r_local + i);
      out->sample_j = (uint32_t)(col0 + c_local + j);
      out->kin = ld_r2(m);
      out->ibs0 = (uint32_t)m.n;
      out->ibs1 = 0;
      out->ibs2 = 0;
    }
  }
}

}  // namespace

hipError_t launch_transpose_sites(const uint64_t *d_bit_set, uint32_t num_stored,
                                  uint32_t words_per_sample, uint32_t num_sites,
                                  uint64_t *d_site_bits, hipStream_t stream) {
  if (num_stored == 0 || num_sites == 0) return hipSuccess;
  TransposeArgs a;
  a.bit_set = d_bit_set;
  a.site_bits = d_site_bits;
  a.num_stored = num_stored;
  a.words_per_sample = words_per_sample;
  a.num_sites = num_sites;
  a.q_words = ld_site_words(num_stored);
  const uint64_t real_words = ((uint64_t)num_sites + 63) / 64;
  a.word_tiles = (uint32_t)((real_words + kTrWords - 1) / kTrWords);
  const uint64_t blocks = (uint64_t)a.word_tiles * ((a.q_words + kTrGroups - 1) / kTrGroups);
  return launch_in_chunks(blocks, kTrThreads, [&](uint64_t done, uint32_t n) {
    a.block_base = done;
    transpose_sites_kernel<<<dim3(n), dim3(kTrThreads), 0, stream>>>(a);
  });
}

hipError_t launch_ld_edges(const uint64_t *d_site_bits, uint32_t num_sites, uint32_t num_stored,
                           uint32_t window, float r2_threshold, const int32_t *d_group,
                           cuking_result *d_records, uint64_t max_records,
                           unsigned long long *d_count, hipStream_t stream) {
  if (num_sites < 2 || num_stored == 0) return hipSuccess;
  LdArgs a;
  a.site_bits = d_site_bits;
  a.group = d_group;
  a.records = d_records;
  a.count = d_count;
  a.max_records = max_records;
  a.num_sites = num_sites;
  a.q_words = ld_site_words(num_stored);
  a.window = window;
  a.r2_threshold = r2_threshold;
  const uint64_t row_tiles = ((uint64_t)num_sites + kLdTile - 1) / kLdTile;
  // the last column a row tile's band reaches is kLdTile - 1 + window - 1 behind its first row
  uint64_t col_tiles = ((uint64_t)kLdTile + window - 2) / kLdTile + 1;
  if (col_tiles > row_tiles) col_tiles = row_tiles;
  a.col_tiles = (uint32_t)col_tiles;
  const uint64_t blocks = row_tiles * col_tiles;
  return launch_in_chunks(blocks, kLdThreads, [&](uint64_t done, uint32_t n) {
    a.block_base = done;
    ld_edges_kernel<<<dim3(n), dim3(kLdThreads), 0, stream>>>(a);
  });
}

}  // namespace cuking
