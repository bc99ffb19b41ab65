// Mendelian errors of trios and duos on the device (include/cuking_amd.h "Mendelian errors" holds
// the contract, king_mendel.h the word masks as code, king_host.cc the host twins that walk the
// same words one by one; DESIGN.md 4.3k the reasons for the shapes): mendel_trios_kernel and
// mendel_site_counts_kernel.
//
// mendel_trios_kernel -- one WAVEFRONT owns one listed trio.  Per step of 64 words (4096 sites)
// lane l loads word 64 step + l of both planes of the child's, the father's and the mother's row
// (coalesced: 512 bytes per plane and step, the access pattern of roh_samples_kernel), forms the
// eight code masks with mendel_code_masks and takes nine population counts -- the eight codes and
// the called sites -- into registers.  With a mask buffer the lane also stores the OR of the eight
// masks, word 64 step + l of the trio's row: 512 contiguous bytes per wavefront and step.  An absent
// sample loads nothing.  Nine integer butterflies over the lanes, and lane 0 stores the 48-byte row.
// No atomics: a row is a function of its three indices and the bitset.
//
// mendel_site_counts_kernel -- the column sums of a mask [T][W], the shape of site_counts_kernel
// with one class.  A lane owns one word column (64 sites) and walks trios, eight at a time through
// the carry-save adder tree of SliceCounter (king_site_qc.h); a wavefront counts at most
// kSiteWaveSamples trios, so there is no flush inside the walk.  At the end every lane takes its
// counter apart bit by bit and adds it to the workgroup's LDS table [site of the word][word column]
// (stride 65: neither those adds nor the reads below conflict), and the workgroup ADDS the non-zero
// entries to the output with integer atomics, 64 contiguous sites per wavefront.  Integer sums: no
// dependence on launch shape or timing.
#include <hip/hip_runtime.h>

#include "king_common.h"
#include "king_device.h"
#include "king_mendel.h"
#include "king_site_qc.h"

namespace cuking {

namespace {

constexpr uint32_t kMendelWaves = 4;  // trios of a workgroup: one per wavefront
constexpr uint32_t kMendelThreads = 64 * kMendelWaves;
constexpr uint32_t kMendelStepWords = 64;  // words per step: one per lane
static_assert(sizeof(cuking_mendel_trio) == 48, "twelve dwords per output row");
static_assert(kMendelNoParent == CUKING_MENDEL_NO_PARENT, "one sentinel");

struct MendelTrioArgs {
  const uint64_t *bits;
  const uint32_t *trios;  // [num_trios][3]: child, father, mother
  cuking_mendel_trio *out;
  uint64_t *error_bits;  // [num_trios][words_per_sample / 2] or nullptr
  uint64_t num_trios;
  uint64_t trio_base;  // first trio of this launch
  uint32_t num_stored, words_per_sample, num_sites;
};

__global__ __launch_bounds__(kMendelThreads) void mendel_trios_kernel(const MendelTrioArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t t = a.trio_base + (uint64_t)blockIdx.x * kMendelWaves + threadIdx.x / 64;
  if (t >= a.num_trios) return;  // (the whole wavefront: there is no barrier below)

  const uint32_t child = a.trios[3 * t], father = a.trios[3 * t + 1],
                 mother = a.trios[3 * t + 2];
  // (NO_PARENT is never below num_stored)
  const bool has_c = child < a.num_stored, has_f = father < a.num_stored,
             has_m = mother < a.num_stored;
  const uint32_t plane_words = a.words_per_sample / 2;
  const uint64_t *row_c = a.bits + (uint64_t)(has_c ? child : 0) * a.words_per_sample;
  const uint64_t *row_f = a.bits + (uint64_t)(has_f ? father : 0) * a.words_per_sample;
  const uint64_t *row_m = a.bits + (uint64_t)(has_m ? mother : 0) * a.words_per_sample;

  uint32_t errors[kMendelCodes] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t called = 0;
  // Without a mask to store the words at or beyond num_sites are nobody's business.
  const uint32_t words =
      a.error_bits != nullptr ? plane_words : (uint32_t)(((uint64_t)a.num_sites + 63) / 64);
  for (uint32_t w0 = 0; w0 < words; w0 += kMendelStepWords) {
    const uint32_t w = w0 + lane;
    const uint64_t valid = ibd_valid_mask(a.num_sites, w);
    // (valid != 0 implies w < plane_words: the call refuses num_sites > 64 plane_words)
    const bool load = valid != 0 && has_c;
    MendelWord c, f, m;
    if (load) c = mendel_word(row_c[w], row_c[plane_words + w], valid);
    if (load && has_f) f = mendel_word(row_f[w], row_f[plane_words + w], valid);
    if (load && has_m) m = mendel_word(row_m[w], row_m[plane_words + w], valid);
    uint64_t code[kMendelCodes];
    mendel_code_masks(f, m, c, code);
    uint64_t any = 0;
#pragma unroll
    for (uint32_t k = 0; k < kMendelCodes; ++k) {
      errors[k] += (uint32_t)__popcll(code[k]);
      any |= code[k];
    }
    called += (uint32_t)__popcll(mendel_called(f, father != kMendelNoParent, m,
                                               mother != kMendelNoParent, c));
    if (a.error_bits != nullptr && w < plane_words) a.error_bits[t * plane_words + w] = any;
  }

  cuking_mendel_trio row;
  row.child = child;
  row.father = father;
  row.mother = mother;
  row.called = ibd_wave_sum(called);
#pragma unroll
  for (uint32_t k = 0; k < kMendelCodes; ++k) row.errors[k] = ibd_wave_sum(errors[k]);
  if (lane == 0) a.out[t] = row;
}

constexpr uint32_t kMendelSiteThreads = 256;  // four wavefronts, one word-column tile
constexpr uint32_t kMendelTileWords = 64;     // word columns of a workgroup
constexpr uint32_t kMendelMinWaveTrios = 64;
constexpr uint32_t kMendelLdsStride = kMendelTileWords + 1;  // (odd: conflict-free both ways)
constexpr uint32_t kMendelTargetBlocks = 2048;               // eight workgroups per CU

struct MendelSiteArgs {
  const uint64_t *error_bits;  // [num_trios][plane_words]
  uint32_t *counts;            // [64 plane_words]
  uint64_t num_trios;
  uint64_t block_base;  // first workgroup of this launch
  uint32_t plane_words;
  uint32_t wave_trios;   // trios a wavefront counts: a multiple of 8, <= kSiteWaveSamples
  uint32_t trio_chunks;  // workgroups per word-column tile
};

__global__ __launch_bounds__(kMendelSiteThreads) void mendel_site_counts_kernel(
    const MendelSiteArgs a) {
  // [site of the word][word column of the tile]
  __shared__ uint32_t table[64 * kMendelLdsStride];
  const uint64_t block = a.block_base + blockIdx.x;
  const uint32_t chunk = (uint32_t)(block % a.trio_chunks);
  const uint32_t tile = (uint32_t)(block / a.trio_chunks);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t word = tile * kMendelTileWords + lane;

  for (uint32_t k = threadIdx.x; k < 64 * kMendelLdsStride; k += kMendelSiteThreads) table[k] = 0;
  __syncthreads();

  // this wavefront's trios
  const uint64_t begin_ =
      ((uint64_t)chunk * (kMendelSiteThreads / 64) + wave) * (uint64_t)a.wave_trios;
  const uint64_t begin = begin_ < a.num_trios ? begin_ : a.num_trios;
  const uint64_t end = a.num_trios - begin < a.wave_trios ? a.num_trios : begin + a.wave_trios;

  if (word < a.plane_words && begin < end) {
    SliceCounter count;
    count.clear();
    const uint64_t *column = a.error_bits + word;
    for (uint64_t t = begin; t < end; t += kSiteGroup) {
      uint64_t x[kSiteGroup];
      // all eight loads in flight before the first is used; a trio past the end adds nothing
#pragma unroll
      for (uint32_t u = 0; u < kSiteGroup; ++u)
        x[u] = t + u < end ? column[(t + u) * a.plane_words] : 0;
      count.add8(x);
    }
    // the counter, bit by bit, into the workgroup's table (lanes: consecutive addresses)
#pragma unroll
    for (uint32_t half = 0; half < 2; ++half) {
      for (uint32_t bit = 0; bit < 32; ++bit) {
        const uint32_t c = count.count(half, bit);
        if (c) atomicAdd(table + (32 * half + bit) * kMendelLdsStride + lane, c);
      }
    }
  }
  __syncthreads();

  // the table to the output: a thread per site
  for (uint32_t k = threadIdx.x; k < kMendelTileWords * 64; k += kMendelSiteThreads) {
    const uint32_t w = k >> 6, bit = k & 63u;
    if (tile * kMendelTileWords + w >= a.plane_words) break;  // (w grows with k)
    const uint32_t c = table[bit * kMendelLdsStride + w];
    if (c) atomicAdd(a.counts + (uint64_t)(tile * kMendelTileWords + w) * 64 + bit, c);
  }
}

}  // namespace

hipError_t launch_mendel_trios(const uint64_t *d_bits, uint32_t num_stored,
                               uint32_t words_per_sample, uint32_t num_sites,
                               const uint32_t *d_trios, uint64_t num_trios,
                               cuking_mendel_trio *d_out, uint64_t *d_error_bits,
                               hipStream_t stream) {
  if (num_trios == 0) return hipSuccess;
  MendelTrioArgs a;
  a.bits = d_bits;
  a.trios = d_trios;
  a.out = d_out;
  a.error_bits = d_error_bits;
  a.num_trios = num_trios;
  a.trio_base = 0;
  a.num_stored = num_stored;
  a.words_per_sample = words_per_sample;
  a.num_sites = num_sites;
  const uint64_t blocks = (num_trios + kMendelWaves - 1) / kMendelWaves;
  return launch_in_chunks(blocks, kMendelThreads, [&](uint64_t done, uint32_t n) {
    a.trio_base = done * kMendelWaves;
    mendel_trios_kernel<<<dim3(n), dim3(kMendelThreads), 0, stream>>>(a);
  });
}

hipError_t launch_mendel_site_counts(const uint64_t *d_error_bits, uint64_t num_trios,
                                     uint32_t plane_words, uint32_t *d_counts,
                                     hipStream_t stream) {
  if (num_trios == 0 || plane_words == 0) return hipSuccess;
  MendelSiteArgs a;
  a.error_bits = d_error_bits;
  a.counts = d_counts;
  a.num_trios = num_trios;
  a.plane_words = plane_words;
  const uint64_t tiles = ((uint64_t)plane_words + kMendelTileWords - 1) / kMendelTileWords;
  // Trio chunks: as long as the counter allows when that still gives the chip enough workgroups,
  // shorter ones (more flushes, more atomics) for a short list -- the rule of launch_site_counts.
  const uint64_t waves = kMendelSiteThreads / 64;
  const uint64_t want_chunks = (kMendelTargetBlocks + tiles - 1) / tiles;
  uint64_t wave = (num_trios + want_chunks * waves - 1) / (want_chunks * waves);
  wave = (wave + kSiteGroup - 1) / kSiteGroup * kSiteGroup;
  if (wave < kMendelMinWaveTrios) wave = kMendelMinWaveTrios;
  if (wave > kSiteWaveSamples) wave = kSiteWaveSamples;
  a.wave_trios = (uint32_t)wave;
  const uint64_t chunks = (num_trios + wave * waves - 1) / (wave * waves);
  a.trio_chunks = (uint32_t)chunks;  // (checked by the caller: num_trios < 2^32)
  const uint64_t blocks = tiles * chunks;
  return launch_in_chunks(blocks, kMendelSiteThreads, [&](uint64_t done, uint32_t n) {
    a.block_base = done;
    mendel_site_counts_kernel<<<dim3(n), dim3(kMendelSiteThreads), 0, stream>>>(a);
  });
}

}  // namespace cuking
