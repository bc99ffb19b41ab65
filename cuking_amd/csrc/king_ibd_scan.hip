// IBD scan of a block on the device (include/cuking_amd.h "IBD scan of a block" holds the
// contract, king_ibd.h the word masks and the segment test as code, king_host.cc the host twin;
// DESIGN.md 4.3j the reasons for the shape): ibd_scan_kernel.
//
// Every pair of a block is scanned for kind-1 segments and only the pairs that have some become
// records.  Where ibd_pairs_kernel (king_ibd.hip) gives a pair to a wavefront and reloads both
// samples for it, this kernel gives a 32 x 32 TILE of pairs to a workgroup of 256 threads:
//
//   stage    per chunk of kScanChunk = 16 words the two planes of the tile's 32 row and 32 column
//            samples go through LDS (16.1 KiB): thread t loads word t % 16 of sample t / 16 +
//            16 k (128 contiguous bytes per sample) and stores it sample-minor, [word][plane]
//            [sample] with one word of padding per chunk word.  A diagonal tile stages its
//            samples once.  The next chunk's words are fetched into registers while this one
//            is scanned.  A word without a site below num_sites is not loaded.
//   scan     thread t owns the 2 x 2 pairs (t / 16 + 16 p, t % 16 + 16 q) and walks the words in
//            order, which is the host twin's loop: per kind and pair it carries prev, open and
//            the IbdKindSums; a close bit in a word that was entered inside a run ends the run
//            [open, ibd_close_last].  No cross-lane traffic.  Along a wavefront t % 16 varies
//            fastest, so the column reads are 16 consecutive 8-byte words and the row reads
//            broadcasts of 2 addresses per half wavefront: no bank conflict on either side.
//   test     almost every closed run is short: ibd_enough_sites first, and only then pos[a] and
//            pos[b] and THE segment test.  valid and the group word depend on the word alone
//            and are the same for the whole workgroup.
//   records  a pair with segments1 >= 1 and length1 >= min_total inside the block (i < j on a
//            diagonal block) is a record: four ballots per wavefront, ONE atomic add on the
//            counter, plain 40-byte stores into the slots below max_records.
// Only the tiles tile_j >= tile_i of a diagonal block are launched (pcrelate_triangle_tile).
// Edge tiles clamp the sample index for their loads and never store for it.  Integers only, no
// scratch.
#include <hip/hip_runtime.h>

#include "king_common.h"
#include "king_device.h"
#include "king_ibd.h"
#include "king_pcrelate.h"

namespace cuking {

namespace {

constexpr uint32_t kScanTile = 32;     // pairs of a workgroup: kScanTile x kScanTile
constexpr uint32_t kScanThreads = 256; // 16 x 16 threads, 2 x 2 pairs each
constexpr uint32_t kScanChunk = 16;    // words per LDS chunk
constexpr uint32_t kScanSamples = 2 * kScanTile;            // rows, then columns
constexpr uint32_t kScanWordStride = 2 * kScanSamples + 1;  // [plane][sample] + 1 word of padding
constexpr uint32_t kScanLoads = kScanSamples * 2 * kScanChunk / kScanThreads;  // per thread: 8
static_assert(kScanThreads == (kScanTile / 2) * (kScanTile / 2), "2 x 2 pairs per thread");
static_assert(kScanChunk * (kScanTile / 2) == kScanThreads, "one word of 16 samples per pass");
static_assert(sizeof(cuking_ibd_pair) == 40, "ten dwords per record");

struct IbdScanArgs {
  const uint64_t *bits;
  const uint64_t *group_bits;
  const uint32_t *pos;  // or nullptr: pos[s] = s
  cuking_ibd_pair *records;
  unsigned long long *count;
  uint64_t max_records, min_total;
  uint64_t tile_base;  // first tile of this launch
  uint64_t tiles_j;    // tiles per row; per side of the triangle on a diagonal block
  uint32_t i_begin, i_end, j_begin, j_end;
  uint32_t diagonal;   // identical ranges: the triangular map and the test i < j
  uint32_t words_per_sample, num_sites, min_sites, min_length;
};

// What a thread carries from word to word for one pair and kind.
struct IbdScanKind {
  uint32_t prev = 0, open = kIbdInherit;
  IbdKindSums sums;
};

// One word of one pair and kind: the body of the host twin's loop.
__device__ __forceinline__ void ibd_scan_word(const IbdScanArgs &a, uint64_t w, uint64_t in,
                                              uint64_t group, IbdScanKind &k) {
  const uint64_t starts = ibd_starts(in, k.prev, group), closes = ibd_closes(in, k.prev, group);
  if (k.prev != 0 && closes != 0) {
    const uint32_t first = k.open, last = ibd_close_last(closes, w);
    if (ibd_enough_sites(first, last, a.min_sites)) {
      const uint32_t pos_a = a.pos != nullptr ? a.pos[first] : first;
      const uint32_t pos_b = a.pos != nullptr ? a.pos[last] : last;
      if (ibd_is_segment(first, last, pos_a, pos_b, a.min_sites, a.min_length))
        k.sums.add(pos_b - pos_a);
    }
  }
  const uint32_t start = ibd_open_start(starts, w);
  if (start != kIbdInherit) k.open = start;
  k.prev = (uint32_t)(in >> 63);
}

__global__ __launch_bounds__(kScanThreads) void ibd_scan_kernel(const IbdScanArgs a) {
  __shared__ uint64_t lds[kScanChunk * kScanWordStride];
  const uint32_t t = threadIdx.x, lane = t & 63u;
  const uint64_t tile = a.tile_base + blockIdx.x;
  uint32_t tile_i, tile_j;
  if (a.diagonal) {
    pcrelate_triangle_tile(a.tiles_j, tile, &tile_i, &tile_j);
  } else {
    tile_i = (uint32_t)(tile / a.tiles_j);
    tile_j = (uint32_t)(tile % a.tiles_j);
  }
  // (tile_i * kScanTile < rows <= 2^32 - 1: the sums below are taken in 64 bits)
  const uint64_t row0 = (uint64_t)a.i_begin + (uint64_t)tile_i * kScanTile;
  const uint64_t col0 = (uint64_t)a.j_begin + (uint64_t)tile_j * kScanTile;
  // A diagonal tile: the columns ARE the rows, staged once.
  const bool same = a.diagonal && tile_i == tile_j;
  const uint32_t staged = same ? kScanTile : kScanSamples;
  const uint32_t col_slot = same ? 0 : kScanTile;

  // ---- staging: word t % 16 of the samples t / 16 + 16 k, both planes
  const uint32_t plane_words = a.words_per_sample / 2;
  const uint32_t st_word = t % kScanChunk, st_sample = t / kScanChunk;
  const uint64_t *src[kScanLoads / 2];
#pragma unroll
  for (uint32_t k = 0; k < kScanLoads / 2; ++k) {
    const uint32_t slot = st_sample + k * (kScanThreads / kScanChunk);
    // (clamped inside the block: an edge tile reads a real sample and never stores for it)
    uint64_t sample = slot < kScanTile ? row0 + slot : col0 + (slot - kScanTile);
    const uint64_t last = slot < kScanTile ? a.i_end - 1 : a.j_end - 1;
    sample = sample < last ? sample : last;
    src[k] = a.bits + sample * a.words_per_sample;
  }
  uint64_t fetched[kScanLoads];
  const auto fetch = [&](uint64_t w0) {
    const uint64_t w = w0 + st_word;
    // (a site below num_sites in word w implies w < plane_words: num_sites <= 64 plane_words)
    const bool load = w * 64 < a.num_sites;
#pragma unroll
    for (uint32_t k = 0; k < kScanLoads / 2; ++k) {
      const bool mine = load && st_sample + k * (kScanThreads / kScanChunk) < staged;
      fetched[2 * k] = mine ? src[k][w] : 0;
      fetched[2 * k + 1] = mine ? src[k][plane_words + w] : 0;
    }
  };
  const auto stage = [&]() {
#pragma unroll
    for (uint32_t k = 0; k < kScanLoads / 2; ++k) {
      const uint32_t slot = st_sample + k * (kScanThreads / kScanChunk);
      lds[st_word * kScanWordStride + slot] = fetched[2 * k];
      lds[st_word * kScanWordStride + kScanSamples + slot] = fetched[2 * k + 1];
    }
  };

  // ---- the scan: pairs (ti + 16 p, tj + 16 q)
  const uint32_t ti = t / (kScanTile / 2), tj = t % (kScanTile / 2);
  IbdScanKind kind1[2][2], kind2[2][2];
  const uint64_t words = ibd_scan_words(a.num_sites);
  fetch(0);
  for (uint64_t w0 = 0; w0 < words; w0 += kScanChunk) {
    __syncthreads();  // (the chunk before has been read)
    stage();
    __syncthreads();
    if (w0 + kScanChunk < words) fetch(w0 + kScanChunk);
    const uint32_t chunk = words - w0 < kScanChunk ? (uint32_t)(words - w0) : kScanChunk;
    for (uint32_t c = 0; c < chunk; ++c) {
      const uint64_t w = w0 + c;
      // (the same for the whole workgroup)
      const uint64_t valid = ibd_valid_mask(a.num_sites, w), group = a.group_bits[w];
      const uint64_t *het = lds + c * kScanWordStride, *hom = het + kScanSamples;
      uint64_t het_i[2], hom_i[2], het_j[2], hom_j[2];
#pragma unroll
      for (uint32_t p = 0; p < 2; ++p) {
        het_i[p] = het[ti + 16 * p];
        hom_i[p] = hom[ti + 16 * p];
        het_j[p] = het[col_slot + tj + 16 * p];
        hom_j[p] = hom[col_slot + tj + 16 * p];
      }
#pragma unroll
      for (uint32_t p = 0; p < 2; ++p)
#pragma unroll
        for (uint32_t q = 0; q < 2; ++q) {
          ibd_scan_word(a, w, valid & ~ibd_opp(het_i[p], hom_i[p], het_j[q], hom_j[q]), group,
                        kind1[p][q]);
          ibd_scan_word(a, w, valid & ~ibd_diff(het_i[p], hom_i[p], het_j[q], hom_j[q]), group,
                        kind2[p][q]);
        }
    }
  }

  // ---- records: the pairs of this wavefront that have something
  uint64_t found[4];
  uint32_t total = 0;
#pragma unroll
  for (uint32_t p = 0; p < 2; ++p)
#pragma unroll
    for (uint32_t q = 0; q < 2; ++q) {
      const uint64_t i = row0 + ti + 16 * p, j = col0 + tj + 16 * q;
      const IbdKindSums &s = kind1[p][q].sums;
      const bool pair = i < a.i_end && j < a.j_end && (!a.diagonal || i < j);
      found[p * 2 + q] = __ballot(pair && s.segments >= 1 && s.length >= a.min_total);
      total += (uint32_t)__popcll(found[p * 2 + q]);
    }
  if (total == 0) return;  // (the same for every lane; no barrier below)
  unsigned long long base = 0;
  if (lane == 0) base = atomicAdd(a.count, (unsigned long long)total);
  const uint32_t base_lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
  const uint32_t base_hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(base >> 32));
  uint64_t slot = ((uint64_t)base_hi << 32) | base_lo;
  const uint64_t below = (1ull << lane) - 1;
#pragma unroll
  for (uint32_t p = 0; p < 2; ++p)
#pragma unroll
    for (uint32_t q = 0; q < 2; ++q) {
      const uint64_t mask = found[p * 2 + q];
      const uint64_t mine = slot + (uint32_t)__popcll(mask & below);
      if (((mask >> lane) & 1ull) && mine < a.max_records) {
        cuking_ibd_pair row;
        row.sample_i = (uint32_t)(row0 + ti + 16 * p);
        row.sample_j = (uint32_t)(col0 + tj + 16 * q);
        row.segments1 = kind1[p][q].sums.segments;
        row.segments2 = kind2[p][q].sums.segments;
        row.length1 = kind1[p][q].sums.length;
        row.length2 = kind2[p][q].sums.length;
        row.longest1 = kind1[p][q].sums.longest;
        row.longest2 = kind2[p][q].sums.longest;
        a.records[mine] = row;
      }
      slot += (uint32_t)__popcll(mask);
    }
}

}  // namespace

hipError_t launch_ibd_scan(const uint64_t *d_bits, uint32_t words_per_sample, uint32_t num_sites,
                           const uint64_t *d_group_bits, const uint32_t *d_pos,
                           uint32_t min_sites, uint32_t min_length,
                           const cuking_submatrix &block, uint64_t min_total,
                           cuking_ibd_pair *d_records, uint64_t max_records,
                           unsigned long long *d_count, hipStream_t stream) {
  const uint32_t rows = block.i_end - block.i_begin, cols = block.j_end - block.j_begin;
  // (without a site no run exists: no record)
  if (rows == 0 || cols == 0 || num_sites == 0) return hipSuccess;
  IbdScanArgs a;
  a.bits = d_bits;
  a.group_bits = d_group_bits;
  a.pos = d_pos;
  a.records = d_records;
  a.count = d_count;
  a.max_records = max_records;
  a.min_total = min_total;
  a.tile_base = 0;
  a.tiles_j = ((uint64_t)cols + kScanTile - 1) / kScanTile;
  a.i_begin = block.i_begin;
  a.i_end = block.i_end;
  a.j_begin = block.j_begin;
  a.j_end = block.j_end;
  a.diagonal = sm_is_diag(block) ? 1u : 0u;
  a.words_per_sample = words_per_sample;
  a.num_sites = num_sites;
  a.min_sites = min_sites;
  a.min_length = min_length;
  const uint64_t tiles_i = ((uint64_t)rows + kScanTile - 1) / kScanTile;
  // (a side of at most 2^27 tiles: pcrelate_triangle_tile's loops make its square root exact)
  const uint64_t tiles = a.diagonal ? pcrelate_triangle_tiles(a.tiles_j) : tiles_i * a.tiles_j;
  return launch_in_chunks(tiles, kScanThreads, [&](uint64_t done, uint32_t n) {
    a.tile_base = done;
    ibd_scan_kernel<<<dim3(n), dim3(kScanThreads), 0, stream>>>(a);
  });
}

}  // namespace cuking
