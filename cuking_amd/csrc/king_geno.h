// Genotype matrix products (include/cuking_amd.h, "Genotype matrix products"): the definitions
// the kernel of king_geno.hip, the host twin of king_host.cc and the tests share, so that they
// cannot drift apart.  Plain C++: hipcc compiles the functions for the device, the sanitizer
// build of the tests (tests/geno_matmul_host_driver.cc) for the host.
//
// Operand.  uint64 bits[num_rows][words_per_row], W = words_per_row / 2, a row is [W het words |
// W hom_var words], column k = bit k & 63 of word k >> 6.  Both bitsets of the library have
// this shape: the sample-major one (rows = samples, W = plane words, columns = sites) and the
// site-major planes of cuking_transpose_sites (rows = sites, W = Q, columns = samples).
//
// Code.  geno_code = het bit + 2 hom_var bit: 0 hom-ref, 1 het, 2 hom-var, 3 missing -- the
// order of the four counts of cuking_site_counts.  The value of an element is table[code],
// with the table row chosen by the column (kGenoTablePerColumn) or by the row
// (kGenoTablePerRow).
//
// Sum.  out[r][c] = sum over k < num_cols of table(r or k)[code(r, k)] * B[k][c].  The device
// accumulates in float32 in ascending k, one fused multiply-add per term (the f32-input MFMA is
// bit for bit a k-ordered fmaf chain); the host twin accumulates in double and rounds once.
// Neither splits the k range: there is no partial-sum scratch and no split threshold, one
// workgroup owns its rows over every column.  Both stay within the bound of a float32
// accumulation of num_cols terms in any order, (num_cols + 2) 2^-24 sum |table B|.
#ifndef CUKING_AMD_KING_GENO_H_
#define CUKING_AMD_KING_GENO_H_

#include <cstddef>
#include <cstdint>

#ifndef CUKING_HD
#ifdef __HIPCC__
#define CUKING_HD __host__ __device__
#else
#define CUKING_HD
#endif
#endif

namespace cuking {

// (CUKING_GENO_RHS_MAX, CUKING_GENO_TABLE_PER_COLUMN, CUKING_GENO_TABLE_PER_ROW)
constexpr uint32_t kGenoRhsMax = 64;
constexpr int kGenoTablePerColumn = 0;
constexpr int kGenoTablePerRow = 1;

// The code of column `bit` (0 .. 63) of one word pair of a row.
CUKING_HD inline uint32_t geno_code(uint64_t het_word, uint64_t hom_word, uint32_t bit) {
  return (uint32_t)((het_word >> bit) & 1u) | ((uint32_t)((hom_word >> bit) & 1u) << 1);
}

CUKING_HD inline bool geno_axis_valid(int table_axis) {
  return table_axis == kGenoTablePerColumn || table_axis == kGenoTablePerRow;
}

}  // namespace cuking

#endif  // CUKING_AMD_KING_GENO_H_
