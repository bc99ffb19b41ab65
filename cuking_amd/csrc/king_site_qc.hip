// Site QC on the device (include/cuking_amd.h "Site QC" holds the contract, king_host.cc the
// site rule and cuking_compact_sites_host, the specification of the compaction; DESIGN.md 4.3b
// the reasons for the shapes): site_counts_kernel, sample_counts_kernel, compact_sites_kernel.
//
// site_counts_kernel -- genotype counts per site over a range of samples, one read of the
// bitset.  A lane owns one word column (64 sites, both planes) and walks samples: the 64 lanes
// of a wavefront read 512 contiguous bytes of a sample's het plane and 512 of its hom_var
// plane.  The three non-trivial classes (het only, hom_var only, both = missing) are counted in
// bit-sliced vertical counters: eight samples go through a carry-save adder tree into the
// planes of weight 1, 2 and 4 (seven adders of five operations for eight inputs), its carry of
// weight 8 ripples into kSiteUpperPlanes higher planes once per eight samples.  A wavefront
// counts at most kSiteWaveSamples samples (the counters hold 2^(3 + kSiteUpperPlanes) - 1), a
// workgroup of four wavefronts four times that: the launch deals sample chunks accordingly, so
// there is no flush inside the walk.  At the end every lane takes its counters apart bit by
// bit and adds them to the workgroup's LDS table [site of the tile][class], laid out so that
// neither those adds nor the reads of the last phase conflict; the workgroup then ADDS the
// table, with hom-ref as the remainder, to the output with integer atomics -- 16 contiguous
// bytes per site, 64 contiguous sites per wavefront.  Integer sums: no dependence on launch
// shape or timing.
//
// sample_counts_kernel -- one wavefront per sample, popcounts of the four classes over the
// words of its row, the last word masked to [0, num_sites), a butterfly over the lanes.
//
// compact_sites_kernel -- per sample a bit compress (pext) of every word by the SAME mask word
// for all samples.  The mask is turned into a table once per call (king_site_qc.h): per input
// word the six move masks of the parallel-suffix compress and the number of kept sites in
// front of it, per output word the input word its first site comes from.  A thread assembles
// output word j of both planes for kCompactRows samples: it walks the input words from
// first_in[j] while their kept sites fall into [64 j, 64 j + 64), compresses each in six
// shift/and/or steps and shifts it into place; empty mask words are passed by without a
// load.  Neighbouring lanes own neighbouring output words of the same samples.  Every output
// word is written once, with a plain store.
#include <hip/hip_runtime.h>

#include "king_common.h"
#include "king_device.h"
#include "king_site_qc.h"

namespace cuking {

namespace {

constexpr uint32_t kSiteThreads = 256;                   // four wavefronts, one word-column tile
constexpr uint32_t kSiteTileWords = 64;                  // word columns of a workgroup
constexpr uint32_t kSiteBlockSamples = kSiteWaveSamples * (kSiteThreads / 64);  // 2016
constexpr uint32_t kSiteMinWaveSamples = 64;
constexpr uint32_t kSiteLdsStride = kSiteTileWords + 1;  // (odd: conflict-free both ways)
constexpr uint32_t kSiteTargetBlocks = 2048;             // eight workgroups per CU

struct SiteCountArgs {
  const uint64_t *bit_set;
  uint32_t *counts;
  uint32_t num_stored, words_per_sample;
  uint32_t wave_samples;   // samples a wavefront counts: a multiple of 8, <= kSiteWaveSamples
  uint32_t sample_chunks;  // workgroups per word-column tile
  uint64_t block_base;     // first workgroup of this launch
};

__global__ __launch_bounds__(kSiteThreads) void site_counts_kernel(const SiteCountArgs a) {
  // [site of the tile's 64 x 64][class 0 het, 1 hom_var, 2 missing], the word column fastest
  __shared__ uint32_t table[64 * 3 * kSiteLdsStride];
  const uint64_t block = a.block_base + blockIdx.x;
  const uint32_t chunk = (uint32_t)(block % a.sample_chunks);
  const uint32_t tile = (uint32_t)(block / a.sample_chunks);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t plane_words = a.words_per_sample / 2;
  const uint32_t word = tile * kSiteTileWords + lane;

  for (uint32_t k = threadIdx.x; k < 64 * 3 * kSiteLdsStride; k += kSiteThreads) table[k] = 0;
  __syncthreads();

  // this workgroup's samples and, of those, this wavefront's
  const uint64_t block_begin = (uint64_t)chunk * a.wave_samples * (kSiteThreads / 64);
  const uint64_t block_end_ = block_begin + (uint64_t)a.wave_samples * (kSiteThreads / 64);
  const uint32_t block_end = block_end_ < a.num_stored ? (uint32_t)block_end_ : a.num_stored;
  const uint64_t begin_ = block_begin + (uint64_t)wave * a.wave_samples;
  const uint32_t begin = begin_ < block_end ? (uint32_t)begin_ : block_end;
  const uint32_t end = block_end - begin < a.wave_samples ? block_end : begin + a.wave_samples;

  if (word < plane_words && begin < end) {
    SliceCounter het, hom, mis;
    het.clear();
    hom.clear();
    mis.clear();
    const uint64_t *column = a.bit_set + word;
    for (uint32_t s = begin; s < end; s += kSiteGroup) {
      uint64_t h[kSiteGroup], m[kSiteGroup];
      // all sixteen loads in flight before the first is used; a sample past the end counts
      // as 00 (hom-ref: no counter moves, and the remainder below does not include it)
#pragma unroll
      for (uint32_t u = 0; u < kSiteGroup; ++u) {
        const bool in = s + u < end;
        const uint64_t *row = column + (uint64_t)(s + u) * a.words_per_sample;
        h[u] = in ? row[0] : 0;
        m[u] = in ? row[plane_words] : 0;
      }
      uint64_t x[kSiteGroup];
#pragma unroll
      for (uint32_t u = 0; u < kSiteGroup; ++u) x[u] = h[u] & ~m[u];
      het.add8(x);
#pragma unroll
      for (uint32_t u = 0; u < kSiteGroup; ++u) x[u] = m[u] & ~h[u];
      hom.add8(x);
#pragma unroll
      for (uint32_t u = 0; u < kSiteGroup; ++u) x[u] = h[u] & m[u];
      mis.add8(x);
    }
    // the counters, bit by bit, into the workgroup's table (lanes: consecutive addresses)
#pragma unroll
    for (uint32_t half = 0; half < 2; ++half) {
      for (uint32_t bit = 0; bit < 32; ++bit) {
        uint32_t *at = table + ((32 * half + bit) * 3) * kSiteLdsStride + lane;
        const uint32_t c0 = het.count(half, bit), c1 = hom.count(half, bit),
                       c2 = mis.count(half, bit);
        if (c0) atomicAdd(at, c0);
        if (c1) atomicAdd(at + kSiteLdsStride, c1);
        if (c2) atomicAdd(at + 2 * kSiteLdsStride, c2);
      }
    }
  }
  __syncthreads();

  // the table to the output: a thread per site, hom-ref = the samples counted less the rest
  const uint32_t counted = block_end > block_begin ? block_end - (uint32_t)block_begin : 0;
  if (counted == 0) return;
  for (uint32_t k = threadIdx.x; k < kSiteTileWords * 64; k += kSiteThreads) {
    const uint32_t w = k >> 6, bit = k & 63u;
    if (tile * kSiteTileWords + w >= plane_words) break;  // (w grows with k)
    const uint32_t *from = table + (bit * 3) * kSiteLdsStride + w;
    const uint32_t c1 = from[0], c2 = from[kSiteLdsStride], c3 = from[2 * kSiteLdsStride];
    uint32_t *out = a.counts + ((uint64_t)(tile * kSiteTileWords + w) * 64 + bit) * 4;
    atomicAdd(out + 0, counted - c1 - c2 - c3);
    if (c1) atomicAdd(out + 1, c1);
    if (c2) atomicAdd(out + 2, c2);
    if (c3) atomicAdd(out + 3, c3);
  }
}

constexpr uint32_t kSampleThreads = 256;  // four samples per workgroup

__global__ __launch_bounds__(kSampleThreads) void sample_counts_kernel(
    const uint64_t *bit_set, uint32_t num_stored, uint32_t words_per_sample, uint32_t num_sites,
    uint32_t *counts, uint64_t block_base) {
  const uint64_t s = (block_base + blockIdx.x) * (kSampleThreads / 64) + (threadIdx.x >> 6);
  if (s >= num_stored) return;  // (whole wavefronts)
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t plane_words = words_per_sample / 2;
  const uint64_t *row = bit_set + s * words_per_sample;
  uint32_t ref = 0, het = 0, hom = 0, mis = 0;
  const uint32_t words = (uint32_t)(((uint64_t)num_sites + 63) / 64);  // <= plane_words
  for (uint32_t w = lane; w < words; w += 64) {
    const uint64_t h = row[w], m = row[plane_words + w];
    const uint32_t left = num_sites - 64 * w;  // > 0
    const uint64_t valid = left >= 64 ? ~0ull : (1ull << left) - 1;
    ref += (uint32_t)__popcll(~h & ~m & valid);
    het += (uint32_t)__popcll(h & ~m & valid);
    hom += (uint32_t)__popcll(m & ~h & valid);
    mis += (uint32_t)__popcll(h & m & valid);
  }
#pragma unroll
  for (uint32_t d = 32; d > 0; d >>= 1) {
    ref += __shfl_xor(ref, d);
    het += __shfl_xor(het, d);
    hom += __shfl_xor(hom, d);
    mis += __shfl_xor(mis, d);
  }
  if (lane == 0) {
    uint32_t *out = counts + s * 4;
    out[0] = ref;
    out[1] = het;
    out[2] = hom;
    out[3] = mis;
  }
}

constexpr uint32_t kCompactThreads = 256;

struct CompactArgs {
  const uint64_t *in;
  uint64_t *out;
  const CompactWord *words;
  const uint32_t *first_in;
  uint32_t num_stored, words_per_sample_in, words_per_sample_out;
  uint32_t kept;
  uint64_t items;       // row groups x output plane words
  uint64_t block_base;  // first workgroup of this launch
};

__global__ __launch_bounds__(kCompactThreads) void compact_sites_kernel(const CompactArgs a) {
  const uint64_t item = (a.block_base + blockIdx.x) * kCompactThreads + threadIdx.x;
  if (item >= a.items) return;
  const uint32_t plane_in = a.words_per_sample_in / 2, plane_out = a.words_per_sample_out / 2;
  const uint32_t j = (uint32_t)(item % plane_out);  // neighbours: neighbouring output words
  const uint64_t s0 = item / plane_out * kCompactRows;
  const uint32_t rows = a.num_stored - s0 < kCompactRows ? (uint32_t)(a.num_stored - s0)
                                                         : kCompactRows;
  uint64_t het[kCompactRows], hom[kCompactRows];
  compact_output_word(a.words, a.first_in, plane_in, a.kept, a.in + s0 * a.words_per_sample_in,
                      a.words_per_sample_in, rows, j, het, hom);
#pragma unroll
  for (uint32_t r = 0; r < kCompactRows; ++r) {
    if (r >= rows) continue;
    uint64_t *dst = a.out + (s0 + r) * a.words_per_sample_out + j;
    dst[0] = het[r];
    dst[plane_out] = hom[r];
  }
}

}  // namespace

uint32_t site_counts_block_samples() { return kSiteBlockSamples; }

hipError_t launch_site_counts(const uint64_t *d_bit_set, uint32_t num_stored,
                              uint32_t words_per_sample, uint32_t *d_counts,
                              hipStream_t stream) {
  if (num_stored == 0) return hipSuccess;
  SiteCountArgs a;
  a.bit_set = d_bit_set;
  a.counts = d_counts;
  a.num_stored = num_stored;
  a.words_per_sample = words_per_sample;
  const uint64_t tiles = ((uint64_t)words_per_sample / 2 + kSiteTileWords - 1) / kSiteTileWords;
  // Sample chunks: as long as the counters allow when that still gives the chip enough
  // workgroups, shorter ones (more flushes, more atomics) for a small cohort.
  const uint64_t want_chunks = (kSiteTargetBlocks + tiles - 1) / tiles;
  uint64_t wave = ((uint64_t)num_stored + want_chunks * 4 - 1) / (want_chunks * 4);
  wave = (wave + kSiteGroup - 1) / kSiteGroup * kSiteGroup;
  if (wave < kSiteMinWaveSamples) wave = kSiteMinWaveSamples;
  if (wave > kSiteWaveSamples) wave = kSiteWaveSamples;
  a.wave_samples = (uint32_t)wave;
  a.sample_chunks = (uint32_t)(((uint64_t)num_stored + wave * 4 - 1) / (wave * 4));
  const uint64_t blocks = tiles * a.sample_chunks;
  return launch_in_chunks(blocks, kSiteThreads, [&](uint64_t done, uint32_t n) {
    a.block_base = done;
    site_counts_kernel<<<dim3(n), dim3(kSiteThreads), 0, stream>>>(a);
  });
}

hipError_t launch_sample_counts(const uint64_t *d_bit_set, uint32_t num_stored,
                                uint32_t words_per_sample, uint32_t num_sites,
                                uint32_t *d_counts, hipStream_t stream) {
  const uint64_t blocks = ((uint64_t)num_stored + kSampleThreads / 64 - 1) / (kSampleThreads / 64);
  return launch_in_chunks(blocks, kSampleThreads, [&](uint64_t done, uint32_t n) {
    sample_counts_kernel<<<dim3(n), dim3(kSampleThreads), 0, stream>>>(
        d_bit_set, num_stored, words_per_sample, num_sites, d_counts, done);
  });
}

hipError_t launch_compact_sites(const uint64_t *d_in, uint32_t num_stored,
                                uint32_t words_per_sample_in, const void *d_table,
                                uint32_t num_kept, uint64_t *d_out,
                                uint32_t words_per_sample_out, hipStream_t stream) {
  if (num_stored == 0) return hipSuccess;
  CompactArgs a;
  a.in = d_in;
  a.out = d_out;
  a.words = static_cast<const CompactWord *>(d_table);
  a.first_in = reinterpret_cast<const uint32_t *>(a.words + words_per_sample_in / 2);
  a.num_stored = num_stored;
  a.words_per_sample_in = words_per_sample_in;
  a.words_per_sample_out = words_per_sample_out;
  a.kept = num_kept;
  a.items = (((uint64_t)num_stored + kCompactRows - 1) / kCompactRows) * (words_per_sample_out / 2);
  const uint64_t blocks = (a.items + kCompactThreads - 1) / kCompactThreads;
  return launch_in_chunks(blocks, kCompactThreads, [&](uint64_t done, uint32_t n) {
    a.block_base = done;
    compact_sites_kernel<<<dim3(n), dim3(kCompactThreads), 0, stream>>>(a);
  });
}

}  // namespace cuking
