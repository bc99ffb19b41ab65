// Internal: what the host-only half of the C ABI (king_host.cc) shares with the
// HIP half (king_abi.hip).
#ifndef CUKING_AMD_KING_HOST_H_
#define CUKING_AMD_KING_HOST_H_

#include "cuking_amd.h"

// Records the calling thread's error message (cuking_last_error) and returns
// `code`.
cuking_status cuking_fail(cuking_status code, const char *fmt, ...)
    __attribute__((format(printf, 2, 3)));
// Argument checks every entry point that takes a block makes.
cuking_status cuking_check_block(const cuking_submatrix *sm, uint32_t words_per_sample);
// Argument checks of cuking_pack_bed_host / cuking_pack_bed_device (include/cuking_amd.h lists
// them); OK says nothing about there being work to do.
cuking_status cuking_check_bed_args(const cuking_submatrix *sm, uint32_t words_per_sample,
                                    const void *bit_set, const void *bed_rows,
                                    uint64_t row_bytes, uint32_t site_begin, uint32_t site_end,
                                    uint32_t num_sites);
// Argument checks of cuking_site_counts / cuking_sample_counts (`what` names the call) and of
// cuking_compact_sites_host / cuking_compact_sites, which also gives the number of kept sites.
cuking_status cuking_check_counts_args(const char *what, const void *bit_set, uint32_t num_stored,
                                       uint32_t words_per_sample, const void *counts);
cuking_status cuking_check_compact_args(const void *in, uint32_t num_stored,
                                        uint32_t words_per_sample_in, const uint64_t *keep,
                                        uint32_t num_sites_in, const void *out,
                                        uint32_t words_per_sample_out, uint32_t *num_kept);
// Argument checks of cuking_transpose_sites_host / cuking_transpose_sites and of
// cuking_ld_edges_host / cuking_ld_edges (include/cuking_amd.h "LD pruning" lists them), and
// the status of an edge count: INVALID_ARGUMENT above 2^30, RESOURCE_EXHAUSTED above
// max_records.
cuking_status cuking_check_transpose_args(const void *bit_set, uint32_t num_stored,
                                          uint32_t words_per_sample, uint32_t num_sites,
                                          const void *site_bits, uint32_t words_per_site_plane);
cuking_status cuking_check_ld_args(const void *site_bits, uint32_t num_stored, uint32_t window,
                                   float r2_threshold, const void *records, uint64_t max_records,
                                   const void *num_records);
cuking_status cuking_ld_count_status(uint64_t count, uint64_t max_records);
// Argument checks of cuking_geno_matmul_host / cuking_geno_matmul (include/cuking_amd.h
// "Genotype matrix products" lists them); OK says nothing about there being work to do.
cuking_status cuking_check_geno_args(const void *bits, uint32_t num_rows, uint32_t words_per_row,
                                     uint32_t num_cols, const void *table, int table_axis,
                                     const void *b, uint32_t ldb, uint32_t num_rhs,
                                     const void *out, uint32_t ldo);
// Argument checks of cuking_pcrelate_matrix_host / cuking_pcrelate_matrix (include/cuking_amd.h
// "PC-Relate" lists them); OK says nothing about there being work to do.
cuking_status cuking_check_pcrelate_args(const void *bits, uint32_t num_stored,
                                         uint32_t words_per_sample, uint32_t num_sites,
                                         const void *x, uint32_t ldx, const void *beta,
                                         uint32_t ldbeta, uint32_t d, float lo, float hi,
                                         const cuking_submatrix *block, const void *out,
                                         uint64_t ldo);
// Argument checks of cuking_pcrelate_records_host / cuking_pcrelate_records (include/cuking_amd.h
// "PC-Relate records" lists them: those of the matrix call through one shared check, then its
// own), and the status of a record count: RESOURCE_EXHAUSTED above max_records.
cuking_status cuking_check_pcrelate_records_args(const void *bits, uint32_t num_stored,
                                                 uint32_t words_per_sample, uint32_t num_sites,
                                                 const void *x, uint32_t ldx, const void *beta,
                                                 uint32_t ldbeta, uint32_t d, float lo, float hi,
                                                 const cuking_submatrix *block, float min_kin,
                                                 const void *records, uint64_t max_records,
                                                 const void *num_records);
cuking_status cuking_pcrelate_count_status(uint64_t count, uint64_t max_records);
// Argument checks of cuking_pcrelate_pairs_host / cuking_pcrelate_pairs (include/cuking_amd.h
// "PC-Relate for listed pairs" lists them); OK says nothing about there being work to do.
cuking_status cuking_check_pcrelate_pairs_args(const void *bits, uint32_t words_per_sample,
                                               uint32_t num_sites, const void *x, uint32_t ldx,
                                               const void *beta, uint32_t ldbeta, uint32_t d,
                                               float lo, float hi, const void *pairs,
                                               uint64_t num_pairs, uint32_t pair_stride,
                                               const void *out);
// Argument checks of cuking_ibd_pairs_host / cuking_ibd_pairs (include/cuking_amd.h "IBD segments
// for listed pairs" lists them; OK says nothing about there being work to do), the check of
// positions on HOST copies of group and pos (FAILED_PRECONDITION names the first site whose
// position decreases inside a group), and the status of a segment count: RESOURCE_EXHAUSTED
// above max_segments.
cuking_status cuking_check_ibd_args(const void *bits, uint32_t words_per_sample,
                                    uint32_t num_sites, uint32_t min_sites, const void *pairs,
                                    uint64_t num_pairs, uint32_t pair_stride, const void *out,
                                    const void *segments, uint64_t max_segments,
                                    const void *num_segments);
cuking_status cuking_check_ibd_positions(const int32_t *group, const uint32_t *pos,
                                         uint32_t num_sites);
cuking_status cuking_ibd_count_status(uint64_t count, uint64_t max_segments);
// The one refusal the bridged calls add: 0 < bridge_sites < 64.
cuking_status cuking_check_ibd_bridge(uint32_t bridge_sites);
// Argument checks of cuking_roh_samples_host / cuking_roh_samples: the two above, for a list of
// samples that may be null and has no stride.
cuking_status cuking_check_roh_args(const void *bits, uint32_t words_per_sample,
                                    uint32_t num_sites, uint32_t min_sites, uint32_t bridge_sites,
                                    uint64_t num_samples, const void *out, const void *segments,
                                    uint64_t max_segments, const void *num_segments);
// Argument checks of cuking_ibd_scan_host / cuking_ibd_scan (include/cuking_amd.h "IBD scan of a
// block" lists them: the block through the check of the PC-Relate records, words_per_sample,
// num_sites and min_sites through cuking_check_ibd_args, then its own; OK says nothing about
// there being work to do), and the status of a record count: RESOURCE_EXHAUSTED above
// max_records.
cuking_status cuking_check_ibd_scan_args(const void *bits, uint32_t num_stored,
                                         uint32_t words_per_sample, uint32_t num_sites,
                                         uint32_t min_sites, const cuking_submatrix *block,
                                         const void *records, uint64_t max_records,
                                         const void *num_records);
cuking_status cuking_ibd_scan_count_status(uint64_t count, uint64_t max_records);
// Argument checks of cuking_mendel_trios_host / cuking_mendel_trios and of
// cuking_mendel_site_counts_host / cuking_mendel_site_counts (include/cuking_amd.h "Mendelian
// errors" lists them); OK says nothing about there being work to do.
cuking_status cuking_check_mendel_args(const void *bits, uint32_t words_per_sample,
                                       uint32_t num_sites, const void *trios, uint64_t num_trios,
                                       const void *out);
cuking_status cuking_check_mendel_site_args(const void *error_bits, uint64_t num_trios,
                                            uint32_t plane_words, const void *counts);
// Argument checks of cuking_hwe_sites_host / cuking_hwe_sites (include/cuking_amd.h
// "Hardy-Weinberg test" lists them); OK says nothing about there being work to do.
cuking_status cuking_check_hwe_args(const void *counts, uint32_t num_sites, uint32_t flags,
                                    const void *p);
// What the PI_HAT calls (include/cuking_amd.h "PI_HAT") check of model and flags.
cuking_status cuking_check_pihat_args(const cuking_pihat_model *model, uint32_t flags);

#endif  // CUKING_AMD_KING_HOST_H_
