// The tile body of the PC-Relate matrix and record kernels (king_pcrelate.hip,
// king_pcrelate_records.hip; DESIGN.md 4.3e the reasons for the shape): ONE function both
// kernels call, so that num and den of a pair are the same two float32 chains and kin the same
// bytes wherever it is computed.  Device code only.
//
// num = sum_s r(i, s) r(j, s), den = sum_s v(i, s) v(j, s): two N x N x S products of matrices
// that exist only as (2-bit genotype, low-rank frequency model) and are expanded in LDS, one
// step of sites at a time, never in memory.  A workgroup of four wavefronts owns a kPcrTile x
// kPcrTile = 128 x 128 tile of the block over EVERY site: the site range is not split, so a sum
// is one chain in ascending s and needs neither scratch nor atomics, and an entry does not
// depend on the block or tile it lies in.  Wavefront w owns the 64 x 64 quadrant (w >> 1, w & 1)
// of the tile: 2 x 2 sub-tiles of 32 x 32, each with one num and one den float32 accumulator of
// the f32-input MFMA v_mfma_f32_32x32x2_f32, which is bit for bit an s-ordered fmaf chain.
//
// Per step of kPcrStep = 32 sites (half a word of each plane):
//   stage    the workgroup copies beta[32][D] into LDS, zeros for sites >= num_sites and columns
//            >= d: a zero row gives mu = 0, which no bound admits, so the tail sites are zero
//            operands, not code paths.
//   expand   thread t owns one sample: t < 128 row t of the tile, t >= 128 column t - 128.  It
//            holds the sample's X row in D registers (zero-padded, statically indexed) and the
//            sample's het and hom_var word; per site it reads the beta row as an LDS broadcast,
//            runs pcrelate_mu and pcrelate_element and writes r and v into LDS [site][sample].
//            A sample beyond the block reads as missing everywhere: r = v = 0.
//   multiply step j of 16 takes sites 2 j + h (h = lane >> 5): A = r or v of the row sample
//            lane & 31 of a sub-tile, B = the same of the column sample.  Rows of the LDS images
//            lie kPcrStride = 288 floats apart: the two half-wavefronts of an operand read rows
//            2 j and 2 j + 1, 288 floats = 32 (mod 64) banks apart.
// What a kernel does with the sums is its epilogue; pcrelate_tile_row / pcrelate_tile_col say
// where the C/D layout put them.
#ifndef CUKING_AMD_KING_PCRELATE_TILE_H_
#define CUKING_AMD_KING_PCRELATE_TILE_H_

#include <hip/hip_runtime.h>

#include "king_common.h"
#include "king_device.h"
#include "king_pcrelate.h"

namespace cuking {

constexpr uint32_t kPcrThreads = 256;
constexpr uint32_t kPcrTile = 128;             // rows and columns of a workgroup's tile
constexpr uint32_t kPcrStep = 32;              // sites per step
constexpr uint32_t kPcrStride = 2 * kPcrTile + 32;  // floats between sites of an LDS image
static_assert(kPcrThreads == 2 * kPcrTile, "one thread per row and per column sample");
static_assert(kPcrStride % 64 == 32, "the two halves of an operand read different banks");

using f32x16 = __attribute__((ext_vector_type(16))) float;

// What the body reads; the kernels' arguments begin with it.
struct PcrTileArgs {
  const uint64_t *bits;
  const float *x;
  const float *beta;
  uint32_t words_per_sample, num_sites, ldx, ldbeta, d;
  uint32_t i_begin, i_end, j_begin, j_end;
  uint32_t tiles_j;  // tiles per row of the rectangular map (per side of a diagonal block)
  float lo, hi;
  uint64_t block_base;  // first workgroup of this launch
};

inline PcrTileArgs pcrelate_tile_args(const uint64_t *d_bits, uint32_t words_per_sample,
                                      uint32_t num_sites, const float *d_x, uint32_t ldx,
                                      const float *d_beta, uint32_t ldbeta, uint32_t d, float lo,
                                      float hi, const cuking_submatrix &block) {
  PcrTileArgs a;
  a.bits = d_bits;
  a.x = d_x;
  a.beta = d_beta;
  a.words_per_sample = words_per_sample;
  a.num_sites = num_sites;
  a.ldx = ldx;
  a.ldbeta = ldbeta;
  a.d = d;
  a.i_begin = block.i_begin;
  a.i_end = block.i_end;
  a.j_begin = block.j_begin;
  a.j_end = block.j_end;
  a.tiles_j = (uint32_t)(((uint64_t)(block.j_end - block.j_begin) + kPcrTile - 1) / kPcrTile);
  a.lo = lo;
  a.hi = hi;
  a.block_base = 0;
  return a;
}

// The C/D layout of a thread's accumulators: register i of sub-tile (p, q) holds the entry at
// this row and this column of the workgroup's tile.
__device__ __forceinline__ uint32_t pcrelate_tile_row(uint32_t p, uint32_t i) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  return (wave >> 1) * 64 + p * 32 + c_row((int)i, lane >> 5);
}
__device__ __forceinline__ uint32_t pcrelate_tile_col(uint32_t q) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  return (wave & 1u) * 64 + q * 32 + (lane & 31u);
}

// num and den of the tile whose first row sample is row0 and first column sample col0, over
// every site.  Called by all kPcrThreads threads of the workgroup (it holds barriers).
template <uint32_t D>
__device__ __forceinline__ void pcrelate_tile_sums(const PcrTileArgs &a, uint64_t row0,
                                                   uint64_t col0, f32x16 (&num)[2][2],
                                                   f32x16 (&den)[2][2]) {
  __shared__ float r_lds[kPcrStep * kPcrStride];
  __shared__ float v_lds[kPcrStep * kPcrStride];
  __shared__ __attribute__((aligned(16))) float beta_lds[kPcrStep * D];
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63u, wave = tid >> 6;
  const uint32_t half = lane >> 5, col = lane & 31u;

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
}

}  // namespace cuking

#endif  // CUKING_AMD_KING_PCRELATE_TILE_H_
