"""cuking_amd: MI355X-native KING-robust kinship (all-pairs popcount path).

Hot path only: bitset pack -> all-pairs AND/popcount kernel -> thresholded
KingResult records, behind the C ABI of include/cuking_amd.h.  The HIP library
is loaded on first use and there is no CPU fallback.
"""
from .api import (DEFAULT_KIN_THRESHOLD, DEFAULT_MAX_RESULTS,  # noqa: F401
                  KING_COUNTS_DTYPE, KING_CUTOFFS, KING_RESULT_DTYPE, CukingError,
                  RelativeCounts, relative_counts,
                  UnrelatedSet, family_members, unrelated_key, unrelated_set, unrelated_set_host,
                  KingContext, KinSummary, ResourceExhaustedError, Submatrix,
                  bytes_per_pair, device_count, kin_matrix, kin_summary, new_host_bitset,
                  pack_bed_host, pack_host,
                  LDPrune, ld_edges_host, ld_priority_host, ld_site_words, transpose_sites_host,
                  geno_matmul_host,
                  SiteQC, compact_sites_host, site_mask_bool, site_mask_host, site_mask_words,
                  HWE_MIDP, hwe_site_mask, hwe_sites_host,
                  padded_sites, sort_results, synth_model_number, synth_models,
                  words_per_sample)
from .pca import PCAResult, hwe_table, pca_host  # noqa: F401
from .pcrelate import (PCRELATE_PAIR_DTYPE, PCRelatePairs, PCRelateRecords,  # noqa: F401
                       PCRelateResult, isaf_fit, pcrelate_host, pcrelate_matrix_host,
                       pcrelate_pairs_host, pcrelate_pairs_raw_host, pcrelate_records_host,
                       pcrelate_records_raw_host)
from .ibd import (IBD_PAIR_DTYPE, IBD_SEGMENT_DTYPE, IBDPairs, genome_length,  # noqa: F401
                  ibd_scan_host, ibd_scan_raw_host, ibd_segments_host, ibd_segments_raw_host)
from .roh import (ROH_SAMPLE_DTYPE, ROHSamples, roh_segments_host,  # noqa: F401
                  roh_segments_raw_host)
from .mendel import (MENDEL_TRIO_DTYPE, NO_PARENT, MendelErrors, candidate_trios,  # noqa: F401
                     mendel_errors_host, mendel_errors_raw_host, trios_from_parents)
from .pihat import (PiHatModel, PiHatRecords, pi_hat_model_host,  # noqa: F401
                    pi_hat_of_records, pi_hat_records_device, pi_hat_records_host)

__version__ = "0.1.0"
