// PC-Relate records on the device (include/cuking_amd.h "PC-Relate records" holds the contract,
// king_pcrelate.h the element functions, the record rule and the tile map as code, king_host.cc
// the specification in executable form; DESIGN.md 4.3g the reasons): pcrelate_records_kernel.
//
// The scan of every pair of a block for kin(i, j) > min_kin, without the matrix.  The per-tile
// body -- the 128 x 128 tile over every site, the 32-site steps, the LDS expansion, the
// v_mfma_f32_32x32x2_f32 accumulators, the templates on D -- is pcrelate_matrix_kernel's
// (king_pcrelate.hip has the description), statement for statement, so that num and den of a
// pair are the same two float32 chains and kin the same bytes as the matrix entry.  It is a
// copy in a file of its own, not a shared function: the matrix kernel's code object stays what
// it was.  Two things differ.
//
//   tile map   an off-diagonal block takes the rectangular map; a diagonal block only its
//              tiles with tile_j >= tile_i, numbered over the triangle
//              (pcrelate_triangle_tile): 2080 workgroups instead of 4096 for 8192 samples.
//   epilogue   each lane tests its 64 entries (inside the block, i < j on a diagonal block,
//              pcrelate_is_record) and keeps a 64-bit mask; the lanes' counts go through a
//              wavefront prefix sum, lane 0 reserves the wavefront's slots with ONE 64-bit
//              atomic add on the record counter -- none when the wavefront has no record --,
//              and the lanes store their records with plain stores while slot < max_records.
//              At min_kin = -inf, where every pair is a record, that is one atomic per 4096
//              pairs.
#include <hip/hip_runtime.h>

#include "king_common.h"
#include "king_device.h"
#include "king_pcrelate.h"

namespace cuking {

namespace {

constexpr uint32_t kPcrThreads = 256;
constexpr uint32_t kPcrTile = 128;             // rows and columns of a workgroup's tile
constexpr uint32_t kPcrStep = 32;              // sites per step
constexpr uint32_t kPcrStride = 2 * kPcrTile + 32;  // floats between sites of an LDS image
static_assert(kPcrThreads == 2 * kPcrTile, "one thread per row and per column sample");
static_assert(kPcrStride % 64 == 32, "the two halves of an operand read different banks");

using f32x16 = __attribute__((ext_vector_type(16))) float;

struct PcrRecordArgs {
  const uint64_t *bits;
  const float *x;
  const float *beta;
  cuking_result *records;
  unsigned long long *count;
  uint64_t max_records;
  uint32_t words_per_sample, num_sites, ldx, ldbeta, d;
  uint32_t i_begin, i_end, j_begin, j_end;
  uint32_t tiles_j;   // tiles per row of the rectangular map; per side of the triangle
  uint32_t diagonal;  // identical ranges: the triangular map and the test i < j
  float lo, hi, min_kin;
  uint64_t block_base;  // first workgroup of this launch
};

template <uint32_t D>
__global__ __launch_bounds__(kPcrThreads, 2) void pcrelate_records_kernel(const PcrRecordArgs a) {
  __shared__ float r_lds[kPcrStep * kPcrStride];
  __shared__ float v_lds[kPcrStep * kPcrStride];
  __shared__ __attribute__((aligned(16))) float beta_lds[kPcrStep * D];
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63u, wave = tid >> 6;
  const uint32_t half = lane >> 5, col = lane & 31u;
  const uint64_t tile = a.block_base + blockIdx.x;
  uint32_t tile_i, tile_j;
  if (a.diagonal) {
    pcrelate_triangle_tile(a.tiles_j, tile, &tile_i, &tile_j);
  } else {
    tile_i = (uint32_t)(tile / a.tiles_j);
    tile_j = (uint32_t)(tile % a.tiles_j);
  }
  // (tile_i * kPcrTile < rows <= 2^32 - 1: the sums below are taken in 64 bits)
  const uint64_t row0 = (uint64_t)a.i_begin + (uint64_t)tile_i * kPcrTile;
  const uint64_t col0 = (uint64_t)a.j_begin + (uint64_t)tile_j * kPcrTile;

  // ---- the sample this thread expands
  const bool is_col = tid >= kPcrTile;
  const uint64_t sample = is_col ? col0 + (tid - kPcrTile) : row0 + tid;
  const bool sample_in = sample < (is_col ? a.j_end : a.i_end);
  const uint32_t plane_words = a.words_per_sample / 2;
  const uint64_t *my_bits = a.bits + (sample_in ? sample : 0) * a.words_per_sample;
  float x[D];
#pragma unroll
  for (uint32_t c = 0; c < D; ++c) x[c] = 0.0f;
  if (sample_in && a.num_sites != 0) {
    const float *xr = a.x + sample * a.ldx;
#pragma unroll
    for (uint32_t c = 0; c < D; ++c)
      if (c < a.d) x[c] = xr[c];
  }

  f32x16 num[2][2], den[2][2];
#pragma unroll
  for (uint32_t p = 0; p < 2; ++p)
#pragma unroll
    for (uint32_t q = 0; q < 2; ++q)
#pragma unroll
      for (uint32_t i = 0; i < 16; ++i) num[p][q][i] = den[p][q][i] = 0.0f;

  const uint32_t a_base = (wave >> 1) * 64 + col;            // row samples of this wavefront
  const uint32_t b_base = kPcrTile + (wave & 1u) * 64 + col;  // column samples

  const uint32_t steps = (uint32_t)(((uint64_t)a.num_sites + kPcrStep - 1) / kPcrStep);
  for (uint32_t w = 0; w < steps; ++w) {
    const uint64_t s0 = (uint64_t)w * kPcrStep;
    // ---- stage beta: loads in flight before the barrier that frees the LDS of the step before
    constexpr uint32_t kItems = kPcrStep * D / kPcrThreads > 0 ? kPcrStep * D / kPcrThreads : 1;
    float bv[kItems];
#pragma unroll
    for (uint32_t i = 0; i < kItems; ++i) {
      const uint32_t idx = i * kPcrThreads + tid;
      const uint64_t s = s0 + idx / D;
      const uint32_t c = idx % D;
      bv[i] = (idx < kPcrStep * D && s < a.num_sites && c < a.d) ? a.beta[s * a.ldbeta + c] : 0.0f;
    }
    // (w >> 1 < plane_words: num_sites <= 64 plane_words)
    const uint32_t shift = (w & 1u) * 32;
    const uint32_t het = sample_in ? (uint32_t)(my_bits[w >> 1] >> shift) : ~0u;
    const uint32_t hom = sample_in ? (uint32_t)(my_bits[plane_words + (w >> 1)] >> shift) : ~0u;
    __syncthreads();  // (the step before has been multiplied)
#pragma unroll
    for (uint32_t i = 0; i < kItems; ++i) {
      const uint32_t idx = i * kPcrThreads + tid;
      if (idx < kPcrStep * D) beta_lds[idx] = bv[i];
    }
    __syncthreads();

    // ---- expand: r and v of this thread's sample at the step's sites
#pragma unroll 4
    for (uint32_t s = 0; s < kPcrStep; ++s) {
      const float mu = pcrelate_mu(x, beta_lds + s * D, D);
      const uint32_t code = geno_code(het, hom, s);
      float r, v;
      pcrelate_element(code, mu, a.lo, a.hi, &r, &v);
      r_lds[s * kPcrStride + tid] = r;
      v_lds[s * kPcrStride + tid] = v;
    }
    __syncthreads();

    // ---- multiply: step j takes sites 2 j + half
    const float *r_row = r_lds + half * kPcrStride;
    const float *v_row = v_lds + half * kPcrStride;
#pragma unroll 4
    for (uint32_t j = 0; j < kPcrStep / 2; ++j) {
      const uint32_t at = 2 * j * kPcrStride;
      const float ra[2] = {r_row[at + a_base], r_row[at + a_base + 32]};
      const float rb[2] = {r_row[at + b_base], r_row[at + b_base + 32]};
      const float va[2] = {v_row[at + a_base], v_row[at + a_base + 32]};
      const float vb[2] = {v_row[at + b_base], v_row[at + b_base + 32]};
#pragma unroll
      for (uint32_t p = 0; p < 2; ++p)
#pragma unroll
        for (uint32_t q = 0; q < 2; ++q) {
          num[p][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(ra[p], rb[q], num[p][q], 0, 0, 0);
          den[p][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(va[p], vb[q], den[p][q], 0, 0, 0);
        }
    }
  }

  // ---- epilogue: the record rule on this lane's 64 entries (bit (p * 2 + q) * 16 + i of the
  // mask: register i of sub-tile (p, q), column lane & 31, row (i & 3) + 8 (i >> 2) + 4 half)
  const uint64_t lane_row0 = row0 + (wave >> 1) * 64 + 4 * half;
  const uint64_t lane_col0 = col0 + (wave & 1u) * 64 + col;
  uint64_t mine = 0;
#pragma unroll
  for (uint32_t p = 0; p < 2; ++p)
#pragma unroll
    for (uint32_t q = 0; q < 2; ++q) {
      const uint64_t j = lane_col0 + q * 32;
#pragma unroll
      for (uint32_t i = 0; i < 16; ++i) {
        const uint64_t r = lane_row0 + p * 32 + (i & 3u) + 8 * (i >> 2);
        const bool pair = r < a.i_end && j < a.j_end && (!a.diagonal || r < j);
        if (pair && pcrelate_is_record(pcrelate_kin(num[p][q][i], den[p][q][i]), a.min_kin))
          mine |= 1ull << ((p * 2 + q) * 16 + i);
      }
    }
  // ---- the wavefront's slots: an inclusive prefix sum of the lanes' counts, one atomic
  const uint32_t count = (uint32_t)__popcll(mine);
  uint32_t upto = count;
#pragma unroll
  for (uint32_t step = 1; step < 64; step *= 2) {
    const uint32_t below = (uint32_t)__shfl_up((int)upto, step, 64);
    if (lane >= step) upto += below;
  }
  const uint32_t total = (uint32_t)__shfl((int)upto, 63, 64);
  if (total == 0) return;  // (the same for every lane)
  unsigned long long base = 0;
  if (lane == 0) base = atomicAdd(a.count, (unsigned long long)total);
  const uint32_t base_lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
  const uint32_t base_hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(base >> 32));
  uint64_t slot = (((uint64_t)base_hi << 32) | base_lo) + (upto - count);
  // ---- plain stores inside the buffer only
#pragma unroll
  for (uint32_t p = 0; p < 2; ++p)
#pragma unroll
    for (uint32_t q = 0; q < 2; ++q) {
      const uint64_t j = lane_col0 + q * 32;
#pragma unroll
      for (uint32_t i = 0; i < 16; ++i) {
        if (!((mine >> ((p * 2 + q) * 16 + i)) & 1ull)) continue;
        if (slot < a.max_records) {
          cuking_result *out = a.records + slot;
          out->sample_i = (uint32_t)(lane_row0 + p * 32 + (i & 3u) + 8 * (i >> 2));
          out->sample_j = (uint32_t)j;
          out->kin = pcrelate_kin(num[p][q][i], den[p][q][i]);
          out->ibs0 = 0;
          out->ibs1 = 0;
          out->ibs2 = 0;
        }
        ++slot;
      }
    }
}

template <uint32_t D>
hipError_t launch_pcr_records(PcrRecordArgs a, uint64_t tiles, hipStream_t stream) {
  const uint64_t cap = max_blocks_per_launch(kPcrThreads);
  for (uint64_t done = 0; done < tiles; done += cap) {
    const uint64_t n = tiles - done < cap ? tiles - done : cap;
    a.block_base = done;
    pcrelate_records_kernel<D><<<dim3((uint32_t)n), dim3(kPcrThreads), 0, stream>>>(a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace

hipError_t launch_pcrelate_records(const uint64_t *d_bits, uint32_t words_per_sample,
                                   uint32_t num_sites, const float *d_x, uint32_t ldx,
                                   const float *d_beta, uint32_t ldbeta, uint32_t d, float lo,
                                   float hi, const cuking_submatrix &block, float min_kin,
                                   cuking_result *d_records, uint64_t max_records,
                                   unsigned long long *d_count, hipStream_t stream) {
  const uint32_t rows = block.i_end - block.i_begin, cols = block.j_end - block.j_begin;
  if (rows == 0 || cols == 0 || num_sites == 0) return hipSuccess;
  PcrRecordArgs a;
  a.bits = d_bits;
  a.x = d_x;
  a.beta = d_beta;
  a.records = d_records;
  a.count = d_count;
  a.max_records = max_records;
  a.words_per_sample = words_per_sample;
  a.num_sites = num_sites;
  a.ldx = ldx;
  a.ldbeta = ldbeta;
  a.d = d;
  a.i_begin = block.i_begin;
  a.i_end = block.i_end;
  a.j_begin = block.j_begin;
  a.j_end = block.j_end;
  a.tiles_j = (uint32_t)(((uint64_t)cols + kPcrTile - 1) / kPcrTile);
  a.diagonal = sm_is_diag(block) ? 1u : 0u;
  a.lo = lo;
  a.hi = hi;
  a.min_kin = min_kin;
  a.block_base = 0;
  const uint64_t tiles_i = ((uint64_t)rows + kPcrTile - 1) / kPcrTile;
  const uint64_t tiles = a.diagonal ? pcrelate_triangle_tiles(a.tiles_j) : tiles_i * a.tiles_j;
  if (d <= 4) return launch_pcr_records<4>(a, tiles, stream);
  if (d <= 8) return launch_pcr_records<8>(a, tiles, stream);
  if (d <= 16) return launch_pcr_records<16>(a, tiles, stream);
  return launch_pcr_records<32>(a, tiles, stream);
}

}  // namespace cuking
