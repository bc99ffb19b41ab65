// PC-Relate on the device (include/cuking_amd.h "PC-Relate" holds the contract, king_pcrelate.h
// the element functions as code, king_host.cc the specification in executable form; DESIGN.md
// 4.3e the reasons for the shape): pcrelate_matrix_kernel.
//
// out[i - i_begin][j - j_begin] = num / (4 den), num = sum_s r(i, s) r(j, s), den = sum_s v(i, s)
// v(j, s): two N x N x S products of matrices that exist only as (2-bit genotype, low-rank
// frequency model) and are expanded in LDS, one step of sites at a time, never in memory.  A
// workgroup of four wavefronts owns a kPcrTile x kPcrTile = 128 x 128 tile of the block over
// EVERY site: the site range is not split, so a sum is one chain in ascending s and needs
// neither scratch nor atomics, and an entry does not depend on the block or tile it lies in.
// Wavefront w owns the 64 x 64 quadrant (w >> 1, w & 1) of the tile: 2 x 2 sub-tiles of 32 x 32,
// each with one num and one den float32 accumulator of the f32-input MFMA
// v_mfma_f32_32x32x2_f32, which is bit for bit an s-ordered fmaf chain.
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
// The epilogue divides and stores with plain stores from the C/D layout (column lane & 31, row
// (i & 3) + 8 (i >> 2) + 4 h of register i); nothing outside the block is written.
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

struct PcrArgs {
  const uint64_t *bits;
  const float *x;
  const float *beta;
  float *out;
  uint64_t ldo;
  uint32_t words_per_sample, num_sites, ldx, ldbeta, d;
  uint32_t i_begin, i_end, j_begin, j_end;
  uint32_t tiles_j;
  float lo, hi;
  uint64_t block_base;  // first workgroup of this launch
};

template <uint32_t D>
__global__ __launch_bounds__(kPcrThreads, 2) void pcrelate_matrix_kernel(const PcrArgs a) {
  __shared__ float r_lds[kPcrStep * kPcrStride];
  __shared__ float v_lds[kPcrStep * kPcrStride];
  __shared__ __attribute__((aligned(16))) float beta_lds[kPcrStep * D];
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63u, wave = tid >> 6;
  const uint32_t half = lane >> 5, col = lane & 31u;
  const uint64_t tile = a.block_base + blockIdx.x;
  const uint32_t tile_i = (uint32_t)(tile / a.tiles_j), tile_j = (uint32_t)(tile % a.tiles_j);
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

  // ---- epilogue: kin = num / (4 den), plain stores inside the block only
#pragma unroll
  for (uint32_t p = 0; p < 2; ++p)
#pragma unroll
    for (uint32_t q = 0; q < 2; ++q) {
      const uint64_t j = col0 + (wave & 1u) * 64 + q * 32 + col;
#pragma unroll
      for (uint32_t i = 0; i < 16; ++i) {
        const uint64_t r = row0 + (wave >> 1) * 64 + p * 32 + (i & 3u) + 8 * (i >> 2) + 4 * half;
        if (r < a.i_end && j < a.j_end)
          a.out[(r - a.i_begin) * a.ldo + (j - a.j_begin)] = pcrelate_kin(num[p][q][i], den[p][q][i]);
      }
    }
}

template <uint32_t D>
hipError_t launch_pcr(PcrArgs a, uint64_t tiles, hipStream_t stream) {
  const uint64_t cap = max_blocks_per_launch(kPcrThreads);
  for (uint64_t done = 0; done < tiles; done += cap) {
    const uint64_t n = tiles - done < cap ? tiles - done : cap;
    a.block_base = done;
    pcrelate_matrix_kernel<D><<<dim3((uint32_t)n), dim3(kPcrThreads), 0, stream>>>(a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace

hipError_t launch_pcrelate_matrix(const uint64_t *d_bits, uint32_t words_per_sample,
                                  uint32_t num_sites, const float *d_x, uint32_t ldx,
                                  const float *d_beta, uint32_t ldbeta, uint32_t d, float lo,
                                  float hi, const cuking_submatrix &block, float *d_out,
                                  uint64_t ldo, hipStream_t stream) {
  const uint32_t rows = block.i_end - block.i_begin, cols = block.j_end - block.j_begin;
  if (rows == 0 || cols == 0) return hipSuccess;
  PcrArgs a;
  a.bits = d_bits;
  a.x = d_x;
  a.beta = d_beta;
  a.out = d_out;
  a.ldo = ldo;
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
  a.lo = lo;
  a.hi = hi;
  a.block_base = 0;
  const uint64_t tiles = (((uint64_t)rows + kPcrTile - 1) / kPcrTile) * a.tiles_j;
  if (d <= 4) return launch_pcr<4>(a, tiles, stream);
  if (d <= 8) return launch_pcr<8>(a, tiles, stream);
  if (d <= 16) return launch_pcr<16>(a, tiles, stream);
  return launch_pcr<32>(a, tiles, stream);
}

}  // namespace cuking
