// PC-Relate on the device (include/cuking_amd.h "PC-Relate" holds the contract, king_pcrelate.h
// the element functions as code, king_host.cc the specification in executable form; DESIGN.md
// 4.3e the reasons for the shape): pcrelate_matrix_kernel.
//
// out[i - i_begin][j - j_begin] = num / (4 den), num = sum_s r(i, s) r(j, s), den = sum_s v(i, s)
// v(j, s).  The sums of a workgroup's 128 x 128 tile are pcrelate_tile_sums (king_pcrelate_tile.h
// has the description: stage, expand, multiply), which the record kernel calls too; what is
// here is the rectangular tile map and the epilogue, which divides and stores with plain stores
// from the C/D layout; nothing outside the block is written.
#include <hip/hip_runtime.h>

#include "king_common.h"
#include "king_device.h"
#include "king_pcrelate.h"
#include "king_pcrelate_tile.h"

namespace cuking {

namespace {

struct PcrArgs {
  PcrTileArgs t;
  float *out;
  uint64_t ldo;
};

template <uint32_t D>
__global__ __launch_bounds__(kPcrThreads, 2) void pcrelate_matrix_kernel(const PcrArgs a) {
  const uint64_t tile = a.t.block_base + blockIdx.x;
  const uint32_t tile_i = (uint32_t)(tile / a.t.tiles_j), tile_j = (uint32_t)(tile % a.t.tiles_j);
  // (tile_i * kPcrTile < rows <= 2^32 - 1: the sums below are taken in 64 bits)
  const uint64_t row0 = (uint64_t)a.t.i_begin + (uint64_t)tile_i * kPcrTile;
  const uint64_t col0 = (uint64_t)a.t.j_begin + (uint64_t)tile_j * kPcrTile;

  f32x16 num[2][2], den[2][2];
  pcrelate_tile_sums<D>(a.t, row0, col0, num, den);

  // ---- epilogue: kin = num / (4 den), plain stores inside the block only
#pragma unroll
  for (uint32_t p = 0; p < 2; ++p)
#pragma unroll
    for (uint32_t q = 0; q < 2; ++q) {
      const uint64_t j = col0 + pcrelate_tile_col(q);
#pragma unroll
      for (uint32_t i = 0; i < 16; ++i) {
        const uint64_t r = row0 + pcrelate_tile_row(p, i);
        if (r < a.t.i_end && j < a.t.j_end)
          a.out[(r - a.t.i_begin) * a.ldo + (j - a.t.j_begin)] =
              pcrelate_kin(num[p][q][i], den[p][q][i]);
      }
    }
}

}  // namespace

hipError_t launch_pcrelate_matrix(const uint64_t *d_bits, uint32_t words_per_sample,
                                  uint32_t num_sites, const float *d_x, uint32_t ldx,
                                  const float *d_beta, uint32_t ldbeta, uint32_t d, float lo,
                                  float hi, const cuking_submatrix &block, float *d_out,
                                  uint64_t ldo, hipStream_t stream) {
  const uint32_t rows = block.i_end - block.i_begin, cols = block.j_end - block.j_begin;
  if (rows == 0 || cols == 0) return hipSuccess;
  PcrArgs a{pcrelate_tile_args(d_bits, words_per_sample, num_sites, d_x, ldx, d_beta, ldbeta, d,
                               lo, hi, block),
            d_out, ldo};
  const uint64_t tiles = (((uint64_t)rows + kPcrTile - 1) / kPcrTile) * a.t.tiles_j;
  return pcrelate_dispatch_columns(d, [&](auto columns) {
    return launch_in_chunks(tiles, kPcrThreads, [&](uint64_t done, uint32_t n) {
      a.t.block_base = done;
      pcrelate_matrix_kernel<decltype(columns)::value>
          <<<dim3(n), dim3(kPcrThreads), 0, stream>>>(a);
    });
  });
}

}  // namespace cuking
