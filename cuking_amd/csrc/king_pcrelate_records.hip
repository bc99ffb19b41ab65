// PC-Relate records on the device (include/cuking_amd.h "PC-Relate records" holds the contract,
// king_pcrelate.h the element functions, the record rule and the tile map as code, king_host.cc
// the specification in executable form; DESIGN.md 4.3g the reasons): pcrelate_records_kernel.
//
// The scan of every pair of a block for kin(i, j) > min_kin, without the matrix.  The sums of a
// workgroup's 128 x 128 tile are pcrelate_tile_sums (king_pcrelate_tile.h), the function
// pcrelate_matrix_kernel calls, so that num and den of a pair are the same two float32 chains
// and kin the same bytes as the matrix entry.  Two things differ.
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
#include "king_pcrelate_tile.h"

namespace cuking {

namespace {

struct PcrRecordArgs {
  PcrTileArgs t;  // (tiles_j: per side of the triangle on a diagonal block)
  cuking_result *records;
  unsigned long long *count;
  uint64_t max_records;
  uint32_t diagonal;  // identical ranges: the triangular map and the test i < j
  float min_kin;
};

// Calls `entry(p, q, i, row, col)` for each of the lane's 64 entries, in the order of the mask
// and of the slots: register i of sub-tile (p, q) is bit (p * 2 + q) * 16 + i.
template <typename Entry>
__device__ __forceinline__ void for_each_entry(uint64_t row0, uint64_t col0, Entry &&entry) {
#pragma unroll
  for (uint32_t p = 0; p < 2; ++p)
#pragma unroll
    for (uint32_t q = 0; q < 2; ++q) {
      const uint64_t j = col0 + pcrelate_tile_col(q);
#pragma unroll
      for (uint32_t i = 0; i < 16; ++i) entry(p, q, i, row0 + pcrelate_tile_row(p, i), j);
    }
}

template <uint32_t D>
__global__ __launch_bounds__(kPcrThreads, 2) void pcrelate_records_kernel(const PcrRecordArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t tile = a.t.block_base + blockIdx.x;
  uint32_t tile_i, tile_j;
  if (a.diagonal) {
    pcrelate_triangle_tile(a.t.tiles_j, tile, &tile_i, &tile_j);
  } else {
    tile_i = (uint32_t)(tile / a.t.tiles_j);
    tile_j = (uint32_t)(tile % a.t.tiles_j);
  }
  // (tile_i * kPcrTile < rows <= 2^32 - 1: the sums below are taken in 64 bits)
  const uint64_t row0 = (uint64_t)a.t.i_begin + (uint64_t)tile_i * kPcrTile;
  const uint64_t col0 = (uint64_t)a.t.j_begin + (uint64_t)tile_j * kPcrTile;

  f32x16 num[2][2], den[2][2];
  pcrelate_tile_sums<D>(a.t, row0, col0, num, den);

  // ---- epilogue: the record rule on this lane's 64 entries
  uint64_t mine = 0;
  for_each_entry(row0, col0, [&](uint32_t p, uint32_t q, uint32_t i, uint64_t r, uint64_t j) {
    const bool pair = r < a.t.i_end && j < a.t.j_end && (!a.diagonal || r < j);
    if (pair && pcrelate_is_record(pcrelate_kin(num[p][q][i], den[p][q][i]), a.min_kin))
      mine |= 1ull << ((p * 2 + q) * 16 + i);
  });
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
  for_each_entry(row0, col0, [&](uint32_t p, uint32_t q, uint32_t i, uint64_t r, uint64_t j) {
    if (!((mine >> ((p * 2 + q) * 16 + i)) & 1ull)) return;
    if (slot < a.max_records) {
      cuking_result *out = a.records + slot;
      out->sample_i = (uint32_t)r;
      out->sample_j = (uint32_t)j;
      out->kin = pcrelate_kin(num[p][q][i], den[p][q][i]);
      out->ibs0 = 0;
      out->ibs1 = 0;
      out->ibs2 = 0;
    }
    ++slot;
  });
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
  PcrRecordArgs a{pcrelate_tile_args(d_bits, words_per_sample, num_sites, d_x, ldx, d_beta,
                                     ldbeta, d, lo, hi, block),
                  d_records, d_count, max_records, sm_is_diag(block) ? 1u : 0u, min_kin};
  const uint64_t tiles_i = ((uint64_t)rows + kPcrTile - 1) / kPcrTile;
  const uint64_t tiles = a.diagonal ? pcrelate_triangle_tiles(a.t.tiles_j) : tiles_i * a.t.tiles_j;
  return pcrelate_dispatch_columns(d, [&](auto columns) {
    return launch_in_chunks(tiles, kPcrThreads, [&](uint64_t done, uint32_t n) {
      a.t.block_base = done;
      pcrelate_records_kernel<decltype(columns)::value>
          <<<dim3(n), dim3(kPcrThreads), 0, stream>>>(a);
    });
  });
}

}  // namespace cuking
