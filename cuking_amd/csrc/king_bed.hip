// pack_bed_kernel: PLINK 1 .bed rows (variant-major, 2 bits per genotype) -> the reference's
// bitset (cuking.cu:507-523), on the device.  include/cuking_amd.h (cuking_pack_bed_device)
// holds the contract, csrc/king_host.cc (cuking_pack_bed_host) the specification in
// executable form; DESIGN.md 4.3a the reasons for the shape.
//
// The job is a bit-matrix transpose of two planes: input [site][sample / 4] bytes, output
// [sample][site / 64] words of het = b0 ^ b1 and hom_var = ~b1.  No atomics, no memset: every
// output word is written once, with a plain store, by the one workgroup that owns it.
//
// One workgroup (4 wavefronts) owns a tile of kBedTileSites x kBedTileSamples genotypes:
//   load       512 row segments of 64 B each go to LDS.  Rows of a .bed start at any byte
//              (row_bytes is odd as often as not, the data sits 3 bytes into the file), so
//              the loads are ALIGNED dwords -- 17 cover a segment -- that v_alignbyte shifts
//              into place; the dword at either end of the buffer, which may reach across it,
//              is put together from byte loads of the bytes inside.  LDS rows are 17 dwords
//              apart: the transposing read below walks down a column without bank conflicts.
//   transpose  a wavefront takes one dword column (16 samples) and walks the tile's eight
//              groups of 64 sites: lane l reads the dword of site 64 g + l, and one wave64
//              ballot per sample and plane IS the output word of that sample and group.
//              Lane 8 k + g keeps the words of samples k and k + 8 of the column.
//   store      per plane and half column one 8-byte store per lane: the 8 lanes of a sample
//              write its 64 contiguous bytes.
// Samples are tiled from the range's start rounded DOWN to a multiple of 4, so a tile's
// segment starts on a byte whether or not the block does; samples outside the range are
// simply not stored.  Sites from site_end on read as "missing" (01 01 01 01), which is
// what the tail of the last word has to hold.
#include <hip/hip_runtime.h>

#include "king_common.h"
#include "king_device.h"

namespace cuking {

namespace {

constexpr uint32_t kBedTileSites = 512;    // 8 output words per sample and plane: 64 B
constexpr uint32_t kBedTileSamples = 256;  // 64 B of every row
constexpr uint32_t kBedRowDwords = kBedTileSamples / 16;  // 16 dwords of 16 samples
constexpr uint32_t kBedLdsStride = kBedRowDwords + 1;     // (odd: conflict-free columns)
constexpr uint32_t kBedThreads = 256;
constexpr uint32_t kBedBatch = 8;                         // rows a thread loads at a time
constexpr uint32_t kBedMissing = 0x55555555u;             // sixteen genotypes of code 01

struct BedArgs {
  const uint8_t *rows;       // row of site_begin
  uint64_t row_bytes;
  uint64_t *bit_set;
  uint32_t words_per_sample;
  uint32_t site_begin, site_end;
  uint32_t word_end;         // words [site_begin / 64, word_end) are written
  // The block's one or two sample ranges: global samples [begin, end) go to stored
  // samples dst + (s - begin); tiles [0, tiles0) belong to range 0.
  uint32_t begin[2], end[2], dst[2];
  uint32_t tiles0, sample_tiles;
  uint64_t tile_base;        // first tile of this launch
};

// Is the aligned dword at p inside [lo, hi)?  Only the first and the last dword of a chunk can
// fail this; those are put together from the bytes inside.
__device__ inline bool dword_inside(const uint8_t *p, const uint8_t *lo, const uint8_t *hi) {
  return p >= lo && p + 4 <= hi;
}
__device__ inline uint32_t load_bytes_inside(const uint8_t *p, const uint8_t *lo,
                                             const uint8_t *hi) {
  uint32_t v = 0;
  for (int k = 0; k < 4; ++k)
    if (p + k >= lo && p + k < hi) v |= (uint32_t)p[k] << (8 * k);
  return v;
}

__global__ __launch_bounds__(kBedThreads) void pack_bed_kernel(const BedArgs a) {
  __shared__ uint32_t tile[kBedTileSites * kBedLdsStride];
  const uint64_t t = a.tile_base + blockIdx.x;
  const uint32_t tx = (uint32_t)(t % a.sample_tiles);   // sample tiles are the fast index:
  const uint32_t ty = (uint32_t)(t / a.sample_tiles);   // neighbours read neighbouring bytes
  const uint32_t range = tx >= a.tiles0 ? 1u : 0u;
  const uint32_t begin = a.begin[range], end = a.end[range];
  // first sample of the tile (a multiple of 4) and first site (a multiple of 512 past site_begin)
  const uint64_t s0 = (uint64_t)(begin & ~3u) + (uint64_t)(tx - (range ? a.tiles0 : 0u)) * kBedTileSamples;
  const uint64_t site0 = (uint64_t)a.site_begin + (uint64_t)ty * kBedTileSites;

  // ---- load: row segments -> LDS --------------------------------------------------------
  {
    const uint8_t *const lo = a.rows;
    const uint8_t *const hi = a.rows + (uint64_t)(a.site_end - a.site_begin) * a.row_bytes;
    const uint32_t j = threadIdx.x & 15u;  // dword of the segment
    // kBedBatch rows per thread at a time: all their loads are in flight before the first
    // is used.
    for (uint32_t rb = threadIdx.x >> 4; rb < kBedTileSites; rb += kBedBatch * (kBedThreads / 16)) {
      uint32_t low[kBedBatch], top[kBedBatch], shift[kBedBatch];
      // this lane's aligned dword j of the segment of row rb + 16 u, and the segment's offset
      // in it; nullptr: no such site in this chunk (the same for the 16 lanes of a row)
      auto dword_of = [&](uint32_t u, uint32_t *offset) -> const uint8_t * {
        const uint64_t site = site0 + rb + u * (kBedThreads / 16);
        if (site >= a.site_end) return nullptr;
        const uint8_t *seg = a.rows + (site - a.site_begin) * a.row_bytes + (s0 >> 2);
        *offset = (uint32_t)(reinterpret_cast<uintptr_t>(seg) & 3u);
        return seg - *offset + 4 * j;
      };
      uint32_t edges = 0;
#pragma unroll
      for (uint32_t u = 0; u < kBedBatch; ++u) {
        low[u] = top[u] = 0;
        shift[u] = 4;
        const uint8_t *p = dword_of(u, &shift[u]);
        if (p == nullptr) continue;
        if (dword_inside(p, lo, hi)) low[u] = *reinterpret_cast<const uint32_t *>(p);
        else edges |= 1u << u;
        if (j != 15u) continue;  // (lane 15 also fetches the 17th dword)
        if (dword_inside(p + 4, lo, hi)) top[u] = *reinterpret_cast<const uint32_t *>(p + 4);
        else edges |= 0x100u << u;
      }
      if (edges != 0) {  // (rare: a dword that reaches across an end of the chunk)
        for (uint32_t u = 0; u < kBedBatch; ++u) {
          uint32_t offset;
          const uint8_t *p = dword_of(u, &offset);
          if (edges & (1u << u)) low[u] = load_bytes_inside(p, lo, hi);
          if (edges & (0x100u << u)) top[u] = load_bytes_inside(p + 4, lo, hi);
        }
      }
#pragma unroll
      for (uint32_t u = 0; u < kBedBatch; ++u) {
        uint32_t high = __shfl_down(low[u], 1, 16);
        if (j == 15u) high = top[u];
        // bytes shift .. shift + 3 of the pair
        const uint32_t v =
            shift[u] < 4 ? __builtin_amdgcn_alignbyte(high, low[u], shift[u]) : kBedMissing;
        tile[(rb + u * (kBedThreads / 16)) * kBedLdsStride + j] = v;
      }
    }
  }
  __syncthreads();

  // ---- transpose and store -------------------------------------------------------------
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t plane_words = a.words_per_sample / 2;
  const uint32_t word0 = (uint32_t)(site0 >> 6);
  // groups of 64 sites of this tile that are written at all (a chunk ends inside the tile)
  const uint32_t groups = a.word_end - word0 < 8u ? a.word_end - word0 : 8u;
  const uint32_t g_mine = lane & 7u;
  for (uint32_t c = wave; c < kBedRowDwords; c += kBedThreads / 64) {
    const uint64_t sc = s0 + 16u * c;  // first sample of the column
    if (sc + 16 <= begin || sc >= end) continue;
    uint64_t het[2] = {0, 0}, hom[2] = {0, 0};
    for (uint32_t g = 0; g < groups; ++g) {
      const uint32_t v = tile[(64u * g + lane) * kBedLdsStride + c];
      const uint32_t x = v ^ (v >> 1);          // bit 2 k: het of sample k
      const uint32_t key = lane - g;            // == 8 k for the lane that keeps (k, g)
#pragma unroll
      for (uint32_t k = 0; k < 16; ++k) {
        const uint64_t h = __ballot((x & (1u << (2 * k))) != 0);
        const uint64_t m = __ballot((v & (2u << (2 * k))) == 0);
        if (key == 8u * (k & 7u)) {
          het[k >> 3] = h;
          hom[k >> 3] = m;
        }
      }
    }
#pragma unroll
    for (uint32_t half = 0; half < 2; ++half) {
      const uint64_t s = sc + 8u * half + (lane >> 3);
      if (g_mine >= groups || s < begin || s >= end) continue;
      uint64_t *dst = a.bit_set + ((uint64_t)a.dst[range] + (s - begin)) * a.words_per_sample +
                      word0 + g_mine;
      dst[0] = het[half];
      dst[plane_words] = hom[half];
    }
  }
}

}  // namespace

hipError_t launch_pack_bed(const cuking_submatrix &sm, uint32_t words_per_sample,
                           uint64_t *d_bit_set, const uint8_t *d_bed_rows, uint64_t row_bytes,
                           uint32_t site_begin, uint32_t site_end, hipStream_t stream) {
  if (site_begin >= site_end || sm_num_samples(sm) == 0) return hipSuccess;
  BedArgs a;
  a.rows = d_bed_rows;
  a.row_bytes = row_bytes;
  a.bit_set = d_bit_set;
  a.words_per_sample = words_per_sample;
  a.site_begin = site_begin;
  a.site_end = site_end;
  a.word_end = (uint32_t)(((uint64_t)site_end + 63) / 64);
  auto tiles_of = [](uint32_t begin, uint32_t end) {
    if (begin >= end) return 0u;
    return (uint32_t)(((uint64_t)end - (begin & ~3u) + kBedTileSamples - 1) / kBedTileSamples);
  };
  a.begin[0] = sm.i_begin;
  a.end[0] = sm.i_end;
  a.dst[0] = 0;
  a.tiles0 = tiles_of(sm.i_begin, sm.i_end);
  // (a diagonal block stores its samples once: no second range)
  const bool two = !sm_is_diag(sm);
  a.begin[1] = two ? sm.j_begin : 0;
  a.end[1] = two ? sm.j_end : 0;
  a.dst[1] = sm_num_rows(sm);
  a.sample_tiles = a.tiles0 + (two ? tiles_of(sm.j_begin, sm.j_end) : 0u);
  const uint64_t site_tiles = ((uint64_t)(site_end - site_begin) + kBedTileSites - 1) / kBedTileSites;
  const uint64_t tiles = site_tiles * a.sample_tiles;
  return launch_in_chunks(tiles, kBedThreads, [&](uint64_t done, uint32_t n) {
    a.tile_base = done;
    pack_bed_kernel<<<dim3(n), dim3(kBedThreads), 0, stream>>>(a);
  });
}

}  // namespace cuking
