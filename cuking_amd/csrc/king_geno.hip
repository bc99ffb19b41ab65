// Genotype matrix products on the device (include/cuking_amd.h "Genotype matrix products" holds
// the contract, king_geno.h the definitions as code, king_host.cc the specification in
// executable form; DESIGN.md 4.3d the reasons for the shape): geno_matmul_kernel.
//
// out[r][c] = sum over k < num_cols of table(r or k)[code(r, k)] * B[k][c], the 2-bit operand
// decoded in registers, never expanded in memory.  A workgroup of four wavefronts owns kGenoRows
// = 128 rows and all (up to 64) right-hand sides, over EVERY column: the k range is not split,
// so the sum of an element is one chain in ascending k and needs neither scratch nor atomics.
// Wavefront v owns rows 32 v .. 32 v + 31 and one or two 32 x 32 float32 accumulators (right-
// hand sides 0 .. 31 and 32 .. 63; the second only when num_rhs > 32) of the f32-input MFMA
// v_mfma_f32_32x32x2_f32, which is bit for bit a k-ordered fmaf chain.
//
// Per step of 64 columns (one word of each plane):
//   stage    the workgroup copies B[64][64] (B[64][32] with one accumulator) into LDS, zeros for
//            columns >= num_cols and right-hand sides >= num_rhs -- the tails are zero operands, not code paths -- and, with a
//            per-column table, table[64][4], zeros for columns >= num_cols.  B's rows lie
//            kGenoBStride = 96 floats apart: the two half-wavefronts of an MFMA operand read
//            rows k and k + 1, 96 floats = 32 banks apart.
//   decode   lane l (row l & 31 of its wavefront, half h = l >> 5) holds its row's het and
//            hom_var word shifted right by h: step j of 32 takes bits 2 j of both (column 2 j +
//            h), geno_code of king_geno.h, and the table value: one LDS read at [column][code]
//            (per column; the four addresses of a half-wavefront are one broadcast) or three
//            selects among four registers (per row).  Rows >= num_rows decode zero words and are
//            not stored.
//   multiply one MFMA per accumulator: A = the table value, B = the staged B[2 j + h][l & 31].
// The epilogue stores out[r][c < num_rhs] with plain stores from the C/D layout (column l & 31,
// row (i & 3) + 8 (i >> 2) + 4 h of register i); nothing else is written.
#include <hip/hip_runtime.h>

#include "king_common.h"
#include "king_device.h"
#include "king_geno.h"

namespace cuking {

namespace {

constexpr uint32_t kGenoThreads = 256;
constexpr uint32_t kGenoRows = 32 * (kGenoThreads / 64);  // 128: 32 per wavefront
constexpr uint32_t kGenoStep = 64;                        // columns per step: one word
constexpr uint32_t kGenoBStride = 96;                     // floats between staged rows of B
static_assert(kGenoRhsMax == 64, "two 32-wide accumulators per wavefront");

using f32x16 = __attribute__((ext_vector_type(16))) float;

struct GenoArgs {
  const uint64_t *bits;
  const float *table;
  const float *b;
  float *out;
  uint32_t num_rows, words_per_row, num_cols, num_rhs, ldb, ldo;
  uint64_t block_base;  // first workgroup of this launch
};

template <bool PER_ROW, bool TWO>
__global__ __launch_bounds__(kGenoThreads) void geno_matmul_kernel(const GenoArgs a) {
  __shared__ float b_lds[kGenoStep * kGenoBStride];
  __shared__ float t_lds[kGenoStep * 4];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t half = lane >> 5, col = lane & 31u;
  const uint64_t row0 = (a.block_base + blockIdx.x) * kGenoRows + wave * 32;
  const uint64_t row = row0 + col;  // the row this lane decodes
  const bool row_in = row < a.num_rows;
  const uint32_t plane_words = a.words_per_row / 2;
  const uint64_t *my_bits = a.bits + (row_in ? row : 0) * a.words_per_row;

  float t0 = 0.f, t1 = 0.f, t2 = 0.f, t3 = 0.f;
  // (num_cols == 0 is a call without operands: table, bits and B may be null, nothing is read)
  if (PER_ROW && row_in && a.num_cols != 0) {
    t0 = a.table[row * 4 + 0];
    t1 = a.table[row * 4 + 1];
    t2 = a.table[row * 4 + 2];
    t3 = a.table[row * 4 + 3];
  }

  f32x16 acc0, acc1;
#pragma unroll
  for (uint32_t i = 0; i < 16; ++i) acc0[i] = acc1[i] = 0.f;

  const uint32_t steps = (uint32_t)(((uint64_t)a.num_cols + kGenoStep - 1) / kGenoStep);
  for (uint32_t w = 0; w < steps; ++w) {
    const uint64_t k0 = (uint64_t)w * kGenoStep;
    // ---- stage: all loads in flight before the barrier that frees the LDS of the step before
    constexpr uint32_t kCols = TWO ? kGenoRhsMax : kGenoRhsMax / 2;   // right-hand sides staged
    constexpr uint32_t kItems = kGenoStep * kCols / kGenoThreads;     // 16 or 8 per thread
    float v[kItems];
#pragma unroll
    for (uint32_t i = 0; i < kItems; ++i) {
      const uint32_t idx = i * kGenoThreads + threadIdx.x;
      const uint64_t k = k0 + idx / kCols;
      const uint32_t c = idx % kCols;
      v[i] = (k < a.num_cols && c < a.num_rhs) ? a.b[k * a.ldb + c] : 0.f;
    }
    float tv = 0.f;
    if (!PER_ROW) {
      const uint64_t k = k0 + threadIdx.x / 4;
      if (k < a.num_cols) tv = a.table[k * 4 + (threadIdx.x & 3u)];
    }
    // (w < steps <= plane_words: num_cols <= 64 plane_words)
    const uint64_t het = (row_in ? my_bits[w] : 0ull) >> half;
    const uint64_t hom = (row_in ? my_bits[plane_words + w] : 0ull) >> half;
    __syncthreads();  // (the step before has been read)
#pragma unroll
    for (uint32_t i = 0; i < kItems; ++i) {
      const uint32_t idx = i * kGenoThreads + threadIdx.x;
      b_lds[(idx / kCols) * kGenoBStride + idx % kCols] = v[i];
    }
    if (!PER_ROW) t_lds[threadIdx.x] = tv;
    __syncthreads();

    // ---- decode and multiply: step j takes column 2 j + half
    const float *b_row = b_lds + half * kGenoBStride + col;
    const float *t_row = t_lds + half * 4;
#pragma unroll
    for (uint32_t j = 0; j < kGenoStep / 2; ++j) {
      const uint32_t code = geno_code(het, hom, 2 * j);
      float av;
      if (PER_ROW)
        av = code == 0 ? t0 : code == 1 ? t1 : code == 2 ? t2 : t3;
      else
        av = t_row[8 * j + code];
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b_row[2 * j * kGenoBStride], acc0, 0, 0, 0);
      if (TWO)
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b_row[2 * j * kGenoBStride + 32], acc1,
                                                    0, 0, 0);
    }
  }

  // ---- epilogue: plain stores of out[r][c < num_rhs]
#pragma unroll
  for (uint32_t i = 0; i < 16; ++i) {
    const uint64_t r = row0 + (i & 3u) + 8 * (i >> 2) + 4 * half;
    if (r >= a.num_rows) continue;
    float *dst = a.out + r * a.ldo;
    if (col < a.num_rhs) dst[col] = acc0[i];
    if (TWO && col + 32 < a.num_rhs) dst[col + 32] = acc1[i];
  }
}

template <bool PER_ROW, bool TWO>
hipError_t launch_geno(GenoArgs a, hipStream_t stream) {
  const uint64_t blocks = ((uint64_t)a.num_rows + kGenoRows - 1) / kGenoRows;
  return launch_in_chunks(blocks, kGenoThreads, [&](uint64_t done, uint32_t n) {
    a.block_base = done;
    geno_matmul_kernel<PER_ROW, TWO><<<dim3(n), dim3(kGenoThreads), 0, stream>>>(a);
  });
}

}  // namespace

hipError_t launch_geno_matmul(const uint64_t *d_bits, uint32_t num_rows, uint32_t words_per_row,
                              uint32_t num_cols, const float *d_table, bool per_row,
                              const float *d_b, uint32_t ldb, uint32_t num_rhs, float *d_out,
                              uint32_t ldo, hipStream_t stream) {
  if (num_rows == 0) return hipSuccess;
  GenoArgs a;
  a.bits = d_bits;
  a.table = d_table;
  a.b = d_b;
  a.out = d_out;
  a.num_rows = num_rows;
  a.words_per_row = words_per_row;
  a.num_cols = num_cols;
  a.num_rhs = num_rhs;
  a.ldb = ldb;
  a.ldo = ldo;
  a.block_base = 0;
  const bool two = num_rhs > 32;
  if (per_row) return two ? launch_geno<true, true>(a, stream) : launch_geno<true, false>(a, stream);
  return two ? launch_geno<false, true>(a, stream) : launch_geno<false, false>(a, stream);
}

}  // namespace cuking
