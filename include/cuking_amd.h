/*
 * cuking_amd.h -- C ABI of the MI355X-native KING hot path.
 *
 * The reference (populationgenomics/cuKING, cuking.cu) has no library or FFI
 * boundary: its one kernel is launched inline from Run() (cuking.cu:734-741).
 * This header is the boundary a maintainer would bind instead.  Each entry
 * point cites the reference lines it replaces.  Conventions:
 *
 *   - extern "C", plain pointers and sizes, POD structs only; no C++ or torch
 *     types cross the boundary.
 *   - every function returns a cuking_status (0 = OK) unless it is a pure
 *     size/index helper; cuking_last_error() gives the message.
 *   - pointers named d_* are DEVICE pointers (hipMalloc'd, or e.g. a torch
 *     tensor's data_ptr()); everything else is host memory owned by the caller.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).
 *     Calls enqueue work on it and return without synchronising unless stated.
 *   - one context per GPU; a context is used by one host thread at a time.
 *   - there is no CPU fallback: without a usable gfx950 device every device
 *     entry point fails with CUKING_ERR_DEVICE.
 */
#ifndef CUKING_AMD_H_
#define CUKING_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CUKING_ABI_VERSION 2

typedef enum cuking_status {
  CUKING_OK = 0,
  CUKING_ERR_INVALID_ARGUMENT = 1,    /* absl::InvalidArgument, cuking.cu:437-462 */
  CUKING_ERR_FAILED_PRECONDITION = 2, /* e.g. bad n_alt_alleles, cuking.cu:698-702 */
  CUKING_ERR_RESOURCE_EXHAUSTED = 3,  /* result overflow, cuking.cu:747-751 */
  CUKING_ERR_OUT_OF_MEMORY = 4,       /* cuking.cu:113-118 */
  CUKING_ERR_DEVICE = 5               /* any HIP failure (unchecked in the reference, :738-744) */
} cuking_status;

/* cuking.cu:129-179 (struct Submatrix): one block of the upper-triangular
 * block matrix of sample pairs.  Samples are stored rows first, then columns;
 * a diagonal block stores its samples once. */
typedef struct cuking_submatrix {
  uint32_t i_begin, i_end; /* sample row range    */
  uint32_t j_begin, j_end; /* sample column range */
} cuking_submatrix;

/* cuking.cu:182-186 (struct KingResult), 24 bytes. */
typedef struct cuking_result {
  uint32_t sample_i, sample_j;
  float kin;
  uint32_t ibs0, ibs1, ibs2;
} cuking_result;

/* The six per-pair sums of cuking.cu:216-240 (diagnostic output only). */
typedef struct cuking_counts {
  uint32_t het_i, het_j, both_het, opposing_hom, concordant_hom, shared;
} cuking_counts;

/* ------------------------------------------------------------------------ */
/* Host-only helpers (no GPU touched).                                       */
/* ------------------------------------------------------------------------ */

/* cuking.cu:130-152 + flag validation :455-462.  Ranges are clamped to
 * num_samples (the reference wraps when block*size > N). */
cuking_status cuking_submatrix_init(cuking_submatrix *sm, uint32_t num_samples,
                                    uint32_t split_factor,
                                    uint32_t shard_index);
uint32_t cuking_submatrix_num_rows(const cuking_submatrix *sm);    /* :154 */
uint32_t cuking_submatrix_num_cols(const cuking_submatrix *sm);    /* :156 */
uint32_t cuking_submatrix_num_samples(const cuking_submatrix *sm); /* :159-162 */
uint32_t cuking_submatrix_contains(const cuking_submatrix *sm, uint32_t index);      /* :165-168 */
uint32_t cuking_submatrix_sample_offset(const cuking_submatrix *sm, uint32_t index); /* :171-175 */
/* Number of (i < j) pairs the block holds = what the kernel evaluates (:199). */
uint64_t cuking_submatrix_num_pairs(const cuking_submatrix *sm);

uint32_t cuking_padded_sites(uint32_t num_sites);     /* :498-500 (x32) */
uint32_t cuking_words_per_sample(uint32_t num_sites); /* :513 */
/* Algorithmic bytes one pair reads: 2 samples x words_per_sample x 8 (:209-224). */
uint64_t cuking_bytes_per_pair(uint32_t words_per_sample);

/* cuking.cu:675-703 + :317-323 on HOST memory: clears bits of an all-ones
 * (cuking.cu:523) bitset for each triple whose sample is in the block.
 * Relaxed atomic ANDs, so concurrent calls on one bitset from several reader
 * threads are safe (cuking.cu:550-553).  FAILED_PRECONDITION for n_alt outside
 * {0,1,2}; INVALID_ARGUMENT for a row_idx outside the padded sites. */
cuking_status cuking_pack_host(const cuking_submatrix *sm,
                               uint32_t words_per_sample, uint64_t *bit_set,
                               const int64_t *row_idx, const int64_t *col_idx,
                               const int32_t *n_alt_alleles,
                               size_t num_triples);

/* Host half of the compact device pack (below): filters triples to the block
 * (cuking.cu:677-679), validates them exactly like cuking_pack_host (same
 * status codes and messages) and writes, for each one kept, its site index and
 * its block-local sample offset (cuking.cu:171-175) with n_alt in bits 30..31:
 * 8 bytes per genotype for the trip to the GPU instead of the 20 of the three
 * Parquet columns.  site / sample_alt hold num_triples entries; *num_out =
 * entries written.  Thread-safe (no shared state). */
cuking_status cuking_narrow_triples(const cuking_submatrix *sm,
                                    uint32_t words_per_sample,
                                    const int64_t *row_idx, const int64_t *col_idx,
                                    const int32_t *n_alt_alleles, size_t num_triples,
                                    uint32_t *site, uint32_t *sample_alt,
                                    size_t *num_out);

/* PLINK 1 binary genotypes (.bed/.bim/.fam), the dense 2-bit form every cohort already exists
 * in and KING itself reads: the way into the bitset without one (row_idx, col_idx,
 * n_alt_alleles) triple per genotype (20 B in Parquet columns, 8 B after
 * cuking_narrow_triples, against 2 bits here).  The .bed is variant-major: 3 magic bytes
 * 6c 1b 01, then for every variant (site) row_bytes = ceil(N / 4) bytes, N = the number of
 * lines of the .fam.  Sample s of a site sits in byte s >> 2, bits 2 (s & 3) and 2 (s & 3) + 1;
 * with v = (byte >> 2 (s & 3)) & 3:
 *     v = 0  homozygous A1   n_alt 2 (A1 counted)   het 0, hom_var 1
 *     v = 1  missing                                het 1, hom_var 1
 *     v = 2  heterozygous    n_alt 1                het 1, hom_var 0
 *     v = 3  homozygous A2   n_alt 0                het 0, hom_var 0
 * i.e. het = b0 XOR b1, hom_var = NOT b1; unused high bits of a row's last byte are ignored,
 * and all four codes are legal: the pack has no data-dependent failure.  Counting A1 rather
 * than A2 is a convention only: all six sums of ComputeKingKernel (cuking.cu:216-240), and so
 * the kinship and IBS0/1/2, are unchanged when the two alleles of a site are swapped
 * (tests/test_bed_host.py proves it on the naive oracle).
 *
 * cuking_pack_bed_host / cuking_pack_bed_device write what cuking_pack_host produces from an
 * all-ones bitset for the triples (site, sample, n_alt) of that table, byte for byte: sample s
 * at bit_set + SampleOffset(s) * words_per_sample, [het | hom_var] planes, every site from
 * num_sites to the end of the plane missing.  bed_rows points at the row of site `site_begin`
 * -- a chunk of the file behind the magic, rows row_bytes apart, NO alignment (row_bytes is any
 * positive value and the data starts at offset 3, so a row may begin at any byte); nothing
 * outside [bed_rows, bed_rows + (site_end - site_begin) * row_bytes) is read.  A call
 * OVERWRITES, for every stored sample of the block (rows, then columns; a diagonal block's
 * samples once), the words [site_begin / 64, ceil(site_end / 64)) of both planes with plain
 * stores, whatever was there; a call with site_end == num_sites thereby also writes every bit
 * from num_sites to the end of the plane as missing.  Chunks that cover [0, num_sites) write
 * every word of the block's rows: no memset is needed, unlike cuking_pack_device.  Rows of
 * other samples and words outside the chunk's range are left alone.
 * INVALID_ARGUMENT, before any device is touched: a null pointer; site_begin not a multiple of
 * 64; site_end neither a multiple of 64 nor num_sites; site_begin > site_end or site_end >
 * num_sites; cuking_words_per_sample(num_sites) != words_per_sample; 4 * row_bytes < j_end (or
 * i_end).  site_begin == site_end returns OK without work, and so does an empty block.  All
 * byte and word offsets are 64-bit (734k samples x 200k sites is a 36.7 GB file).
 * cuking_bed_check (FAILED_PRECONDITION, one message each): bytes 0-1 are not 6c 1b -- not a
 * PLINK .bed; a third byte of 00 -- sample-major, not supported; file_bytes != 3 + num_sites *
 * row_bytes -- with both numbers in the message.
 * Out of scope: the C++ `cuking` binary; .pgen, VCF and sample-major .bed; reading per rank
 * instead of on rank 0; site or sample filtering while loading. */
uint64_t cuking_bed_row_bytes(uint32_t num_samples_total); /* ceil(N / 4) */
cuking_status cuking_bed_check(const uint8_t magic[3], uint64_t file_bytes,
                               uint32_t num_samples_total, uint32_t num_sites);
cuking_status cuking_pack_bed_host(const cuking_submatrix *sm, uint32_t words_per_sample,
                                   uint64_t *bit_set, const uint8_t *bed_rows,
                                   uint64_t row_bytes, uint32_t site_begin,
                                   uint32_t site_end, uint32_t num_sites);

/* Message of the calling thread's most recent failing call ("" if none). */
const char *cuking_last_error(void);
uint32_t cuking_abi_version(void);

/* ------------------------------------------------------------------------ */
/* Device context and memory.                                                */
/* ------------------------------------------------------------------------ */
typedef struct cuking_ctx cuking_ctx;

int cuking_device_count(void);
/* Binds a context to HIP device `device` (must be gfx950). */
cuking_status cuking_ctx_create(int device, cuking_ctx **out);
void cuking_ctx_destroy(cuking_ctx *ctx);

/* Explicit device memory for hosts without their own allocator (replaces
 * cudaMallocManaged, cuking.cu:109-120: no managed memory on the hot path). */
cuking_status cuking_device_alloc(cuking_ctx *ctx, size_t bytes, void **d_ptr);
cuking_status cuking_device_free(cuking_ctx *ctx, void *d_ptr);
cuking_status cuking_memset_async(cuking_ctx *ctx, void *d_ptr, int byte_value,
                                  size_t bytes, void *stream);
cuking_status cuking_copy_to_device(cuking_ctx *ctx, void *d_dst,
                                    const void *src, size_t bytes, void *stream);
cuking_status cuking_copy_to_host(cuking_ctx *ctx, void *dst, const void *d_src,
                                  size_t bytes, void *stream);
cuking_status cuking_stream_synchronize(cuking_ctx *ctx, void *stream);
/* Extra streams for hosts without their own (e.g. one per Parquet reader
 * thread).  The memory, copy, stream, cuking_pack_device and cuking_pack_bed_device entry
 * points may be called from several host threads at once, each on its own stream; the
 * compute / prepare / timing entry points need one caller at a time. */
cuking_status cuking_stream_create(cuking_ctx *ctx, void **stream);
cuking_status cuking_stream_destroy(cuking_ctx *ctx, void *stream);
/* Events, for hosts that pipeline several staging buffers through one stream
 * (wait for ONE earlier piece of work instead of the whole stream). */
cuking_status cuking_event_create(cuking_ctx *ctx, void **event);
cuking_status cuking_event_record(cuking_ctx *ctx, void *event, void *stream);
cuking_status cuking_event_synchronize(cuking_ctx *ctx, void *event);
cuking_status cuking_event_destroy(cuking_ctx *ctx, void *event);
/* Page-locked host memory for staging buffers. */
cuking_status cuking_host_alloc(cuking_ctx *ctx, size_t bytes, void **ptr);
cuking_status cuking_host_free(cuking_ctx *ctx, void *ptr);

/* ------------------------------------------------------------------------ */
/* The hot path.                                                             */
/* ------------------------------------------------------------------------ */

/* Pack on the device (cuking.cu:675-703 as a kernel): d_bit_set must already
 * be all ones (cuking.cu:523; cuking_memset_async(.., 0xFF, ..)).  Triples
 * live in device memory.  *d_status (one u32, zeroed by the caller) receives
 * a bit mask: 1 = n_alt outside {0,1,2}, 2 = row_idx out of range. */
cuking_status cuking_pack_device(cuking_ctx *ctx, const cuking_submatrix *sm,
                                 uint32_t words_per_sample, uint64_t *d_bit_set,
                                 const int64_t *d_row_idx,
                                 const int64_t *d_col_idx,
                                 const int32_t *d_n_alt_alleles,
                                 size_t num_triples, uint32_t *d_status,
                                 void *stream);

/* The same for triples prepared by cuking_narrow_triples (device copies of its
 * two output arrays).  *d_status as above (2 also flags a sample offset outside
 * the block). */
cuking_status cuking_pack_device_compact(cuking_ctx *ctx, const cuking_submatrix *sm,
                                         uint32_t words_per_sample,
                                         uint64_t *d_bit_set, const uint32_t *d_site,
                                         const uint32_t *d_sample_alt,
                                         size_t num_triples, uint32_t *d_status,
                                         void *stream);

/* cuking_pack_bed_host (above: format, mapping, semantics and refused arguments) as a kernel:
 * a two-plane bit transpose through LDS, no atomics (csrc/king_bed.hip).  d_bed_rows is a
 * chunk of the file's rows in DEVICE memory, at any alignment.  Asynchronous on `stream`; like
 * cuking_pack_device it may be issued from several host threads, each on its own stream:
 * chunks write disjoint words. */
cuking_status cuking_pack_bed_device(cuking_ctx *ctx, const cuking_submatrix *sm,
                                     uint32_t words_per_sample, uint64_t *d_bit_set,
                                     const uint8_t *d_bed_rows, uint64_t row_bytes,
                                     uint32_t site_begin, uint32_t site_end,
                                     uint32_t num_sites, void *stream);

/* Which device kernel evaluates the pairs. */
typedef enum cuking_kernel {
  CUKING_KERNEL_TILED = 0,  /* LDS-staged tile kernels: matrix-core variant (default) or VALU popcount variants */
  CUKING_KERNEL_STREAM = 1  /* one pair per wavefront, wave-level reductions */
} cuking_kernel;
cuking_status cuking_ctx_set_kernel(cuking_ctx *ctx, cuking_kernel kernel);
/* Options of a context, each an int64 (cuking_ctx_set_option refuses unknown keys and
 * values out of range; cuking_ctx_get_option reads every key below).  Results do not
 * depend on any of them.  Tuning knobs of the tiled kernel:
 *   "variant"        compiled kernel shape, 0 .. cuking_num_variants()-1 (default also
 *                    from env CUKING_AMD_VARIANT); 0..4 are VALU AND/popcount shapes, 5,
 *                    6 and 7 the matrix-core kernels: 5 = five plane products on the
 *                    reference's two bit planes, 6 = four plane products on one fp4 code
 *                    per site, 7 = the default: ONE plane product per pair as a rigorous
 *                    upper bound on kinship, and the reference's exact sums for the few
 *                    pairs that bound lets through (one wavefront per candidate pair;
 *                    quadrants with many candidates go to kernel 6) -- same records for
 *                    any data, the bound only decides who computes a pair exactly.  It
 *                    applies to the lean form with 0 < kin_threshold < 1/2; otherwise, and
 *                    for the diagnostic counts, variant 7 runs kernel 6 on the quadrants
 *                    of its tiles.  7 has 256-sample tiles, all others 128 or 64
 *                    (cuking_tile_samples).  6 and 7 serve bitsets below 2^22 sites and
 *                    hand wider ones to 5, which hands bitsets from 2^24 sites on to VALU
 *                    shape 2; the tile edge stays the context variant's.
 *   "band_rows"      tile-rows per scheduling band, 1..64, 0 = chosen by block size (default).
 *   "counts_mode"    0 = lean: four sums per pair in the main loop, the hom/hom count behind
 *                    IBS2 recounted only for emitted pairs; 1 = full: all five sums for
 *                    every pair; -1 = automatic (default): lean when kin_threshold >
 *                    c / sqrt(sites), c = 2.05 (1.6 for the VALU variants), i.e. when few
 *                    pairs are expected to pass.
 *   "split_wgs"      matrix-core variants: short launches cut their remainder of tiles into
 *                    this many equal pieces, 0..4096, default one per CU, 0 = never.
 *   "xcd_swizzle"    matrix-core variants: the workgroups resident on one XCD hold
 *                    consecutive tiles of the band order -- 2 = patches of 32 tiles dealt
 *                    round-robin to the XCDs (default), 1 = one contiguous chunk per XCD,
 *                    0 = off.
 *   "dyn_tail_tiles" matrix-core variants: launches of at least this many tiles hand their
 *                    last ~6 % out through a counter instead of by workgroup index, so that
 *                    the XCDs, which differ by 2-3 %, finish together; default 16384,
 *                    0 = never.
 *   "reuse_prepared" 0 (default) / 1: see cuking_invalidate below.
 * Variant 7 (the filter):
 *   "filter_sort"        0 / 1 (default) / 2: which conversions sort the samples by their
 *                        share of missing calls (see cuking_tile_bounds below).
 *   "filter_lazy_codes"  1 (default): kernel 6's codes are converted only when a launch hands
 *                        it something; 0: with every conversion.
 *   "filter_site_order"  the layout's SITES sorted by what they add to X of unrelated pairs, so
 *                        that tiles leave at an earlier check (the share comes from the
 *                        cohort's measured curve): -1 (default) whole-block conversions of
 *                        blocks of at least 24576 tiles with
 *                        check points, and of those only where the curve forecasts the check
 *                        at least 2/64 of the k-steps earlier than stored order has it at
 *                        the converting call's threshold (a "no" is trusted for the next 15
 *                        conversions of the same block at that threshold; a call at another
 *                        threshold decides and converts again); 0 never; 1 every whole-block
 *                        conversion, its tiles not rotated; 2 is 1 with the head lap: where
 *                        "filter_rotate" would rotate a stored-order layout, a tile starts
 *                        where the tiles of its XCD are INSIDE the head of the order (the
 *                        sites in front of its check), wraps at the head's end and is checked
 *                        after one lap -- the same check on the same counts as 1, so the same
 *                        tiles leave and the same records come out.  -1 takes the lap
 *                        wherever it takes the order.  A launch with a forecast check, a
 *                        forced "filter_check1" entry, no share from the curve or a head
 *                        shorter than "filter_rotate_min_steps" takes no lap: its tiles are
 *                        not rotated.  Bitsets beyond 262,144 sites and the ranges of
 *                        cuking_prepare_samples keep stored order.
 *                        Cost: a conversion that builds the curve waits
 *                        for the stream once to read it (counted in "host_syncs"), and a
 *                        layout that takes the order keeps a second copy of the bitset in
 *                        the stream's scratch for the life of the context (2.5 GB at 100k x
 *                        100k), allocated by that conversion: cuking_ctx_reserve does not
 *                        cover it, so the first such call may allocate and wait.
 *                        Read-only: "site_order_on" (the prepared layout took the order),
 *                        "site_order_share" / "site_order_stored_share" (the share in front
 *                        of an unrotated tile's check, in 64ths, by the curve and by stored
 *                        order's rule as the last such conversion forecast them; 0 = none),
 *                        "site_order_sigma_e6".
 *   "filter_site_gather" the kernel that writes that second copy: -1 (default) a workgroup
 *                        stages 4 samples in LDS, a byte per site, where the sites fit beside
 *                        the wavefronts' tiles (up to 153,472 sites), else 2 samples, a
 *                        nibble per site (every width the order serves), and assembles the
 *                        output words by bit-matrix transposes; 0 the earlier kernel, one
 *                        ballot per output word and plane; 4 / 2 force a form (4: the
 *                        conversion is refused where it does not fit).  The same bytes
 *                        either way.
 *   "filter_check0"      forecast check at an eighth of the sites: 0 off, 1 (default) for
 *                        launches of fewer than 16 rounds, 2 always.
 *   "filter_check1"      rigorous check inside the k loop: 0 off, 1 (default) the entry of
 *                        the share menu picked from threshold and cohort, 2 + k (k = 1..7):
 *                        entry k forced (2, entry 0, is the forecast's: refused).
 *   "filter_check_emit"  live pairs per quadrant a tile may hand to the candidate list at
 *                        the rigorous check and leave anyway, 0..255, default 64.
 *   "filter_rotate"      rotated tiles: 0 off, 1 (default) a tile starts where the tiles of
 *                        its XCD are; 2 (a phase per tile) and 3 + j (phase j, j < 128) are
 *                        test hooks.
 *   "filter_rotate_min_steps", "filter_rotate_min_tiles"
 *                        bitsets of fewer k-steps of 256 sites (default 128) and launches of
 *                        fewer tiles (default 2048) are not rotated.
 * Test hooks that force paths ordinary cohorts do not take:
 *   "filter_site_order_min_tiles"  the tile count from which "filter_site_order" -1 builds a
 *                            curve, default 24576.
 *   "filter_quadrant_cap"    candidates per 128 x 128 quadrant beyond which the quadrant
 *                            goes to kernel 6, 0..16384, default 384.
 *   "filter_cand_cap"        entries of the candidate list per launch chunk, default 2^25.
 *   "filter_split_min_steps" k-steps of 256 sites a piece of a short launch's remainder
 *                            must have, 1..4096, default 8.
 *   "max_launch_blocks"      PROCESS-WIDE: workgroups per launch at most, 0 = the hardware's
 *                            limit (default).
 *   "filter_check_min_steps" PROCESS-WIDE: bitsets of fewer k-steps get no check points,
 *                            4..2^20, default 64.
 * Read-only (cuking_ctx_get_option): the counters "workspace_allocations", "host_syncs"
 * and "conversions_skipped" (see cuking_ctx_reserve and cuking_invalidate below), and diagnostics of variant 7
 * summed over the context's streams, which WAIT for the device: "filter_candidates"
 * (pairs its bound has let through to the exact recount so far), "filter_dense_quadrants"
 * (128 x 128 quadrants it has handed to kernel 6 so far), "filter_early_exits" (tiles that
 * left at the rigorous check), "filter_rotated_tiles" (tiles that started at another phase
 * than the first) and "filter_step_ticks16" (the 100 MHz counter's ticks per k-step x 16
 * as the tiles of the last launch chunk measured them; 0 = none did). */
cuking_status cuking_ctx_set_option(cuking_ctx *ctx, const char *key,
                                    int64_t value);
cuking_status cuking_ctx_get_option(const cuking_ctx *ctx, const char *key,
                                    int64_t *value);
int cuking_num_variants(void);
const char *cuking_variant_name(int variant);

/* ComputeKingKernel (cuking.cu:191-314) with its launch (:725-741): same
 * arguments, same meaning.  For every pair (i < j) of the block computes the
 * six masked popcount sums over d_bit_sets (layout cuking.cu:507-523: sample
 * s at d_bit_sets + SampleOffset(s) * words_per_sample, [het | hom_var]
 * planes), the float32 kinship (:289-294), and appends a cuking_result for
 * each pair with kin > kin_threshold (strict) at slot atomicAdd(d_result_index)
 * if that slot < max_results, else sets *d_result_overflow = 1 (:297-313).
 * d_result_index and d_result_overflow are NOT reset by the call (the caller
 * zeroes them, like cuking.cu:721-722), so several calls may append to one
 * buffer.  Record order is unspecified (sort afterwards, :761-765).
 * Asynchronous on `stream`.
 *
 * Numerics contract.  The sums, IBS0/1/2 and het counts are exact integers for
 * any width.  kin = fl32(0.5f + fl32(num / den)) with the IEEE-correct divide.
 * Below 2^22 sites (4,194,304; every BASELINE config is <= 200,000) every
 * partial sum of num = 2 bh - 4 opp - hi - hj is an integer below 2^24, so the
 * value is the same for every association order and every FMA contraction a
 * compiler may apply to cuking.cu:291-294: bit-exact against the reference.
 * (Variant 6 evaluates num as the integer hi + hj - 2 dd + 2 q, dd =
 * sites where both samples are defined, q = concordant - opposing homozygous
 * sites: the same integer, so the same float, below 2^22 sites; it is not used
 * beyond.  The default variant's records come from the reference's own six
 * sums and float expression, evaluated for every pair its bound admits; the
 * bound carries a margin for both float32 roundings (csrc/king_filter.hip).)
 * From 2^22 sites on, this library evaluates the expression left to
 * right with one float32 rounding per operation (no contraction); a reference
 * build that fuses multiply-adds may differ there in the last bit.  The
 * matrix-core variants count in float32 and serve bitsets up to 2^24 sites; wider
 * ones take a VALU variant automatically (same records).
 *
 * Streams.  The compute / prepare entry points convert the bitset into a
 * kernel-internal layout held by the context.  Calls on different streams of
 * one context are ordered by the library where a conversion would overwrite
 * what an earlier call's kernel may still read (event waits, no host
 * synchronisation); concurrent kernels only arise from
 * cuking_compute_king_rect launches on different streams. */
cuking_status cuking_compute_king(cuking_ctx *ctx, const cuking_submatrix *sm,
                                  uint32_t words_per_sample,
                                  const uint64_t *d_bit_sets,
                                  float kin_threshold, uint32_t max_results,
                                  cuking_result *d_results,
                                  uint32_t *d_result_index,
                                  uint32_t *d_result_overflow, void *stream);

/* Pair-space sharding inside one block (replaces multi-VM --split_factor
 * fan-out, cloud_batch_submit.py:45,73, for the GPUs of one node): the tiled
 * kernel enumerates the block's pairs as cuking_num_tiles() independent
 * square tiles; a rank evaluates tiles [tile_begin, tile_end).  The union of
 * disjoint ranges covering [0, num_tiles) equals cuking_compute_king(). */
uint64_t cuking_num_tiles(const cuking_ctx *ctx, const cuking_submatrix *sm);
uint32_t cuking_tile_samples(const cuking_ctx *ctx); /* samples per tile edge */
/* Which tile of the block tile index `tile` is: rows [*row_begin, *row_end)
 * x columns [*col_begin, *col_end) in global sample indices (clamped to the
 * block).  Host-only; lets a scheduler reason about the samples a tile range
 * touches.  The bounds are in LAYOUT order: the default kernel lays a block's samples
 * out sorted by their share of missing calls (option "filter_sort", default 1: whole-
 * block conversions; samples of equal share -- an ordinary cohort: all of them -- keep
 * their stored order), so in a cohort with low-call-rate samples the samples behind a
 * tile are not the ones these bounds name; the union over all tiles is the block either
 * way.  A caller that needs sample-accurate tiles sets "filter_sort" to 0. */
cuking_status cuking_tile_bounds(const cuking_ctx *ctx,
                                 const cuking_submatrix *sm, uint64_t tile,
                                 uint32_t *row_begin, uint32_t *row_end,
                                 uint32_t *col_begin, uint32_t *col_end);
/* (ctx may be NULL for these three: the default kernel shape is assumed.) */
cuking_status cuking_compute_king_tiles(
    cuking_ctx *ctx, const cuking_submatrix *sm, uint32_t words_per_sample,
    const uint64_t *d_bit_sets, uint64_t tile_begin, uint64_t tile_end,
    float kin_threshold, uint32_t max_results, cuking_result *d_results,
    uint32_t *d_result_index, uint32_t *d_result_overflow, void *stream);

/* The schedules of one block over the GPUs of a node (host arithmetic only; the
 * reference fans shards out over VMs instead: cloud_batch_submit.py:45,73).  ONE
 * implementation (cuking_amd/host/schedule.h) behind the C++ host `cuking --num_gpus=N`
 * and, through these entry points, the Python driver cuking_amd/dist.py.
 *   tile partition   contiguous ranges of the tile enumeration, equal or in proportion
 *                    to per-rank weights: out[2 r], out[2 r + 1] = rank r's [begin, end)
 *   chunk ranges     ascending tile-aligned sample chunks of the staged broadcast:
 *                    out[2 c], out[2 c + 1]; returns the number of chunks (<= num_chunks)
 *   staged steps     what rank `rank` does per chunk (tile rows dealt round-robin): six
 *                    words per chunk -- chunk begin, chunk end, has_rect, row begin, row
 *                    end, row step (samples); returns the number of chunks */
void cuking_schedule_tile_partition(uint64_t num_tiles, uint32_t world, uint64_t *out);
cuking_status cuking_schedule_weighted_tile_partition(uint64_t num_tiles, const double *weights,
                                                      uint32_t world, uint64_t *out);
uint64_t cuking_schedule_calibration_tiles(uint64_t num_tiles, uint32_t world);
uint32_t cuking_schedule_chunk_ranges(uint32_t num_samples, uint32_t tile, uint32_t num_chunks,
                                      uint32_t *out);
uint32_t cuking_schedule_staged_steps(uint32_t num_samples, uint32_t tile, uint32_t world,
                                      uint32_t rank, uint32_t num_chunks, uint32_t *out);

/* Staged form of the same operator for a DIAGONAL block (rows == columns),
 * used when the bitset arrives in pieces (e.g. a chunked RCCL broadcast):
 * cuking_prepare_samples() converts samples [sample_begin, sample_end) (global
 * indices, tile aligned except at the block end) into the context's kernel
 * layout; cuking_compute_king_rect() then evaluates the pairs (i < j) of rows
 * x columns [col_begin, col_end) whose samples have all been prepared, where
 * the rows are the tile rows starting at row_begin, row_begin + row_step, ...
 * below row_end (row_step = 0 or the tile edge: every row of the range; a
 * multiple of the tile edge: every n-th tile row, which is how the GPUs of a
 * node share the rows round-robin).  Rectangles that tile the upper triangle reproduce
 * cuking_compute_king() exactly.  Both are asynchronous on `stream`; kernels
 * of different rectangles may run concurrently on different streams (they only
 * read the prepared layout and append atomically). */
cuking_status cuking_prepare_samples(cuking_ctx *ctx, const cuking_submatrix *sm,
                                     uint32_t words_per_sample,
                                     const uint64_t *d_bit_sets,
                                     uint32_t sample_begin, uint32_t sample_end,
                                     void *stream);
cuking_status cuking_compute_king_rect(
    cuking_ctx *ctx, const cuking_submatrix *sm, uint32_t words_per_sample,
    const uint64_t *d_bit_sets, uint32_t row_begin, uint32_t row_end,
    uint32_t row_step, uint32_t col_begin, uint32_t col_end, float kin_threshold,
    uint32_t max_results, cuking_result *d_results, uint32_t *d_result_index,
    uint32_t *d_result_overflow, void *stream);

/* Sizes the context's workspace for `sm` up front: the kernel-internal layout
 * of the block (cuking.cu:513-523 sizes the reference's one buffer the same
 * way, before anything runs), the tile enumeration's prefix table and, for each
 * of the `num_streams` (<= 8) streams named, the remainder-split slab of the
 * matrix-core kernel.  Afterwards the compute / prepare calls for this block
 * (or a smaller one) on those streams allocate nothing and never wait for the
 * device -- which a host that drives several GPUs from one process needs once
 * collectives are in flight (host/multi_gpu.cc reserves before its first
 * broadcast).  May synchronise the device itself.  The context's
 * "workspace_allocations" / "host_syncs" options (cuking_ctx_get_option) count
 * the allocations and host-side waits made on behalf of the workspace so far. */
cuking_status cuking_ctx_reserve(cuking_ctx *ctx, const cuking_submatrix *sm,
                                 uint32_t words_per_sample, void *const *streams,
                                 size_t num_streams);

/* With the option "reuse_prepared" = 1 a compute / prepare call whose block,
 * width, kernel shape and bitset POINTER equal those of the layout the
 * workspace already holds launches the pair kernel only (the conversion is
 * 1.7 % of a 10k x 100k-site call).  The host thereby promises not to rewrite
 * that bitset in place without calling cuking_invalidate() before the next
 * compute call.  Default 0: like ComputeKingKernel (cuking.cu:191-195), every
 * call reads whatever the bitset holds when it runs. */
cuking_status cuking_invalidate(cuking_ctx *ctx);

/* Diagnostic: the six sums of every pair, no threshold.  d_counts holds
 * NumRows x NumCols records, pair (i, j) at [(i - i_begin) * NumCols +
 * (j - j_begin)]; entries with i >= j are left untouched. */
cuking_status cuking_compute_counts(cuking_ctx *ctx, const cuking_submatrix *sm,
                                    uint32_t words_per_sample,
                                    const uint64_t *d_bit_sets,
                                    cuking_counts *d_counts, void *stream);

/* Dense kinship matrix: the float32 kinship of EVERY pair of the block, no threshold and
 * no records (what hl.king returns, for PC-AiR style partitioning, for looking at the
 * kinship distribution before choosing a threshold).  Pair (i, j) goes to
 * d_kin[(i - i_begin) * ld + (j - j_begin)]; `ld` is the row pitch in ELEMENTS, at least
 * NumCols (all index arithmetic is 64-bit).  The value is the numerics contract's kin above
 * for the pair's exact integer sums -- bit for bit what a record of cuking_compute_king
 * carries, including -inf and NaN when one of the samples has no het site.
 *   CUKING_KIN_UPPER      an off-diagonal block: every entry is written.  A diagonal block:
 *                         the entries with i < j; those with i >= j are left untouched
 *                         (like cuking_compute_counts).
 *   CUKING_KIN_SYMMETRIC  diagonal blocks only: [j][i] = [i][j] as well (a small kernel
 *                         behind the pair kernel, on the same stream), and the diagonal
 *                         holds what the expression gives for (i, i): 0.5 for a sample with
 *                         a het site, NaN otherwise.
 * INVALID_ARGUMENT for a null pointer, ld < NumCols, unknown flags, SYMMETRIC on an
 * off-diagonal block or with a tile range; an empty block returns OK.  The matrix depends
 * on no option and on neither cuking_kernel; entries land at the STORED samples' positions
 * whatever "filter_sort" says (a dense call converts an unsorted layout; the next call of
 * the other kind converts again).  The cost does not depend on the data: contexts of
 * variant 6 and 7 run the four-product matrix-core kernel with an epilogue that stores the
 * float (variant 7 on the quadrants of its tiles); the other variants, the stream kernel
 * and bitsets from 2^22 sites on store it from their full forms.  Asynchronous on `stream`;
 * workspace, stream ordering and "reuse_prepared" as for the other compute entry points.
 * The tile form follows cuking_compute_king_tiles: a range writes exactly the entries of
 * its tiles, disjoint ranges covering [0, num_tiles) equal the whole call.
 * Out of scope: the C++ `cuking` binary, assembling one matrix from several GPUs,
 * IBS0/1/2 matrices (the lean form does not hold the hom/hom count) and half-precision
 * output.  The matrix is 4 B x NumRows x NumCols: 40 GB for a 100k-sample diagonal block;
 * larger cohorts go block by block (cuking_submatrix_init with a split factor). */
#define CUKING_KIN_UPPER     0u  /* entries with i >= j are left untouched */
#define CUKING_KIN_SYMMETRIC 1u  /* diagonal block only: mirrored, diagonal filled */
cuking_status cuking_compute_kin_matrix(cuking_ctx *ctx, const cuking_submatrix *sm,
                                        uint32_t words_per_sample,
                                        const uint64_t *d_bit_sets, float *d_kin,
                                        uint64_t ld, uint32_t flags, void *stream);
cuking_status cuking_compute_kin_matrix_tiles(cuking_ctx *ctx, const cuking_submatrix *sm,
                                              uint32_t words_per_sample,
                                              const uint64_t *d_bit_sets,
                                              uint64_t tile_begin, uint64_t tile_end,
                                              float *d_kin, uint64_t ld, uint32_t flags,
                                              void *stream);

/* Kinship summary: the histogram of the float32 kinship of EVERY pair of the block and every
 * sample's nearest relative, without the matrix and without a threshold -- what the look at
 * the kinship distribution before choosing a threshold needs at sizes where the matrix (4 B x
 * NumRows x NumCols) no longer fits, and where duplicate detection, "drop anyone related to
 * anyone" and PC-AiR style partitioning start.  The output does not grow with the pair count.
 *
 * Histogram: cuking_kin_bins {lo, hi, num_bins}, lo < hi, both finite, 1 <= num_bins <=
 * CUKING_KIN_BINS_MAX; d_hist holds num_bins + 3 (cuking_kin_hist_slots) uint64 slots.  The
 * slot of a kinship `kin` is DEFINED by these float32 operations, one rounding each, nothing
 * fused (cuking_kin_bin_slot evaluates exactly this on the host):
 *     scale = (float)num_bins / (hi - lo)        once per call, on the host
 *     kin is NaN                  -> slot num_bins + 2   NAN
 *     kin < lo                    -> slot 0              UNDER (-inf as well)
 *     t = (kin - lo) * scale
 *     !(t < (float)num_bins)      -> slot num_bins + 1   OVER (+inf, kin >= hi)
 *     otherwise                   -> slot 1 + (uint32_t)t
 * The nominal edges lo + b (hi - lo) / num_bins are approximate: a kinship within a rounding
 * of one may be counted on either side; the expression is the contract.  With hi = 0.5 exact
 * duplicates (kin 0.5) land in OVER.
 *
 * Nearest relative: one uint64 key per sample, d_best[cuking_submatrix_sample_offset(s)]
 * (cuking_submatrix_num_samples keys: rows first, then columns, a diagonal block's samples
 * once).  High word: the order-preserving map of the kinship's bits (bits ^ 0x80000000 for a
 * non-negative float, ~bits for a negative one); low word: ~partner, the partner's GLOBAL
 * sample index -- under an unsigned maximum the larger kinship wins, among equal kinships the
 * lower partner.  A NaN kinship never makes a key; key 0 = no partner with a defined kinship
 * (no real key is 0: -inf maps to the high word 0x007FFFFF).  cuking_kin_best_key builds a
 * key (0 for NaN), cuking_kin_best_decode takes one apart (returns 0 for key 0, else 1).
 *
 * cuking_compute_kin_summary counts every pair the block holds exactly once ((i < j) on a
 * diagonal block, every (i, j) on an off-diagonal one: cuking_submatrix_num_pairs): pair
 * (i, j) adds 1 to its slot of d_hist, raises d_best[offset(i)] to at least key(kin, j) and
 * d_best[offset(j)] to at least key(kin, i).  Both outputs ACCUMULATE, like d_result_index:
 * the call resets neither, the caller zeroes them; calls over disjoint tile ranges (the tiles
 * form follows cuking_compute_king_tiles), on one GPU or several, add up to the whole call --
 * histograms merge by sum, keys by maximum.  Either of d_hist / d_best may be NULL (bins may
 * be NULL when d_hist is).  The kinship is the numerics contract's kin above for the pair's
 * exact integer sums, bit for bit what a record or a matrix entry carries, -inf and NaN
 * included; the result depends on no tuning option, and entries sit at the STORED samples'
 * positions (the call converts the unsorted layout of the dense matrix; the next thresholded
 * call converts again).  The cost does not depend on the data: the lean matrix-core k loop
 * with an epilogue that reduces the kinship of a tile's pairs in LDS and merges with one
 * 64-bit atomic per non-empty slot and key.
 * INVALID_ARGUMENT, before any device is touched: a null context, submatrix or bitset; both
 * outputs NULL; d_hist without bins; num_bins 0 or above CUKING_KIN_BINS_MAX; bounds that are
 * not finite or not lo < hi; a bad tile range; a context that is not the tiled kernel with
 * variant 5, 6 or 7, and bitsets from 2^24 sites on (the VALU and stream kernels have no
 * summary form -- one atomic per pair would be a trap at the sizes this call is for).  An
 * empty block returns OK.  Asynchronous on `stream`; workspace, stream ordering and
 * "reuse_prepared" as for the other compute entry points.
 * Out of scope: the C++ `cuking` binary, merging across ranks (the tiles form and the merge
 * rules make it possible), IBS0/1/2 summaries.  (Per-sample relative counts at thresholds:
 * cuking_compute_relative_counts below.) */
#define CUKING_KIN_BINS_MAX 4096u
typedef struct cuking_kin_bins {
  float lo, hi;
  uint32_t num_bins;
} cuking_kin_bins;
/* Host-only (cuking_kin_bin_slot: 0xFFFFFFFF for bins the compute call would refuse). */
uint32_t cuking_kin_hist_slots(uint32_t num_bins);
uint32_t cuking_kin_bin_slot(const cuking_kin_bins *bins, float kin);
uint64_t cuking_kin_best_key(float kin, uint32_t partner);
uint32_t cuking_kin_best_decode(uint64_t key, float *kin, uint32_t *partner);
cuking_status cuking_compute_kin_summary(cuking_ctx *ctx, const cuking_submatrix *sm,
                                         uint32_t words_per_sample,
                                         const uint64_t *d_bit_sets,
                                         const cuking_kin_bins *bins, uint64_t *d_hist,
                                         uint64_t *d_best, void *stream);
cuking_status cuking_compute_kin_summary_tiles(cuking_ctx *ctx, const cuking_submatrix *sm,
                                               uint32_t words_per_sample,
                                               const uint64_t *d_bit_sets,
                                               uint64_t tile_begin, uint64_t tile_end,
                                               const cuking_kin_bins *bins, uint64_t *d_hist,
                                               uint64_t *d_best, void *stream);

/* Relative counts: for every sample of the block, how many partners it has in each band of a
 * few kinship thresholds -- what "drop samples with too many relatives", ordering a maximal-
 * independent-set pruning by degree and sorting a cohort into duplicate / 1st / 2nd / 3rd
 * degree partners at the KING cut-offs (0.354, 0.177, 0.0884, 0.0442) need, and the exact
 * max_results of a following cuking_compute_king.  No records, no buffer that can overflow.
 *
 * Thresholds: a HOST array of 1 .. CUKING_REL_THRESHOLDS_MAX finite float32 values, strictly
 * ascending.  The BAND of a kinship is the largest t with kin > thresholds[t]: a strict
 * float32 comparison, the one a record's `kin > kin_threshold` makes; 0xFFFFFFFF = none (NaN
 * and -inf never get a band).  cuking_rel_band evaluates the rule on the host (0xFFFFFFFF
 * also for thresholds the compute call would refuse).
 *
 * d_counts[cuking_submatrix_sample_offset(s) * num_thresholds + t] (uint32,
 * cuking_submatrix_num_samples x num_thresholds entries: rows first, then columns, a diagonal
 * block's samples once) = the number of partners of stored sample s whose kinship with it
 * falls in band t.  Every pair the block holds is counted once (cuking_submatrix_num_pairs):
 * a pair in band t adds 1 at both its samples.  "Partners with kin > thresholds[t]" are the
 * suffix sums over t, taken on the host.  The output ACCUMULATES, like d_hist and
 * d_result_index: the call does not reset it, the caller zeroes it; calls over disjoint tile
 * ranges (the tiles form follows cuking_compute_king_tiles) add up to the whole call.  Entries
 * sit at the STORED samples' positions whatever "filter_sort" says.
 *
 * The value counted is the numerics contract's kin above, bit for bit what a record carries:
 * for every t, the suffix-summed count of a sample equals the number of records of
 * cuking_compute_king(kin_threshold = thresholds[t]) that name it, and the column sum (halved
 * on a diagonal block; over the rows of an off-diagonal one) is that call's record count.  The
 * result depends on no tuning option.
 *
 * Cost: that of cuking_compute_king at thresholds[0], less the records -- the same layout
 * (sorted, with the filter's statistics: with "reuse_prepared" a count call followed by a
 * record call on the same bitset converts once), the same filter kernel and bound where 0 <
 * thresholds[0] < 1/2 on a context of variant 7, and counting forms of the kernels behind it
 * that skip the 24-byte record and the hom/hom recount: one atomic per end of a pair above
 * thresholds[0], nothing for the others.
 * INVALID_ARGUMENT, before any device is touched: a null context, submatrix, bitset,
 * thresholds or d_counts; num_thresholds 0 or above CUKING_REL_THRESHOLDS_MAX; thresholds that
 * are not finite or not strictly ascending; a bad tile range; a context that is not the tiled
 * kernel with variant 5, 6 or 7, and bitsets from 2^24 sites on.  An empty block returns OK.
 * Asynchronous on `stream` (the thresholds are read before the call returns); workspace,
 * stream ordering, cuking_ctx_reserve and "reuse_prepared" as for the other compute entry
 * points.
 * Out of scope: the C++ `cuking` binary; merging across ranks (the tiles form and the merge
 * rule -- counts add -- make it possible); splitting first degree into parent-child and
 * siblings by IBS0 (the counting forms do not hold the hom/hom count); the VALU and stream
 * kernels. */
#define CUKING_REL_THRESHOLDS_MAX 8u
/* Host-only. */
uint32_t cuking_rel_band(const float *thresholds, uint32_t num_thresholds, float kin);
cuking_status cuking_compute_relative_counts(cuking_ctx *ctx, const cuking_submatrix *sm,
                                             uint32_t words_per_sample,
                                             const uint64_t *d_bit_sets,
                                             const float *thresholds, uint32_t num_thresholds,
                                             uint32_t *d_counts, void *stream);
cuking_status cuking_compute_relative_counts_tiles(cuking_ctx *ctx, const cuking_submatrix *sm,
                                                   uint32_t words_per_sample,
                                                   const uint64_t *d_bit_sets,
                                                   uint64_t tile_begin, uint64_t tile_end,
                                                   const float *thresholds,
                                                   uint32_t num_thresholds, uint32_t *d_counts,
                                                   void *stream);

/* Unrelated set and families from the records: which samples to keep so that no two kept
 * samples are related, and which samples form one family -- the step behind the records, on the
 * buffer cuking_compute_king wrote, without a trip to the host (24 B per record otherwise).
 *
 * Edge: a record with kin > prune_threshold (strict float32, the comparison a record itself
 * makes; NaN is refused, -inf takes every record with a defined kinship above -inf).  Records
 * may repeat (the concatenated buffers of several shards); repeats count once.  EVERY record
 * must satisfy sample_i < sample_j < num_samples: one that does not makes the call fail with
 * CUKING_ERR_INVALID_ARGUMENT, and nothing outside the per-sample arrays is read or written
 * because of it (the outputs are then unspecified).
 * Priority key: one uint64 per sample, cuking_unrelated_key(priority[s], s) =
 * cuking_kin_best_key(priority[s], s) for a number -- the higher priority wins, among equals
 * the LOWER sample index --; a NaN priority is lower than every number: high word 0, low word
 * ~s.  Without priorities (NULL): -(float)degree[s], degree = the number of DISTINCT partners
 * of s among the edges -- fewer relatives first.
 * Unrelated set: the samples taken in descending key order; keep[s] = 1 if none of its
 * neighbours was kept before it, else 0 -- the lexicographically first maximal independent set
 * of that order; a sample without edges is kept.  A function of the edge SET and the keys
 * alone: not of record order, repeats, launch shape or the timing of atomics.  This is
 * deliberately NOT Hail's maximal_independent_set, which removes the currently highest-degree
 * vertex and recomputes the degrees: that has no parallel form with a unique answer.
 * Family: family[s] = the lowest sample index of the connected component of s in the edge
 * graph (s itself without edges).  family may be NULL.
 *
 * cuking_unrelated_set_host: host memory, no GPU -- deduplicate, sort by key, the sequential
 * greedy, union-find: the specification in executable form.
 * cuking_unrelated_set: d_records exactly what cuking_compute_king appended, num_records from
 * its *d_result_index (at most 2^30; num_samples at most 2^31); d_priority (num_samples
 * floats) may be NULL; d_keep num_samples bytes, d_family num_samples words or NULL.  *rounds
 * (HOST memory, may be NULL) receives the number of rounds of the parallel greedy that had a
 * live edge (at most num_samples).  The call WAITS for `stream`: it reads a few control words
 * back per batch of rounds.  Its workspace -- 16 B per record, 20 B per sample and, without
 * priorities, 8 B x the power of two from 2 x num_records on for the duplicate removal --
 * belongs to the context's per-stream cache and is sized once per call; nothing is allocated
 * inside the round loop.  Results depend on no option.
 * Out of scope: the C++ `cuking` binary, merging across ranks, Hail's dynamic-degree
 * heuristic. */
uint64_t cuking_unrelated_key(float priority, uint32_t sample);
cuking_status cuking_unrelated_set_host(const cuking_result *records, uint64_t num_records,
                                        uint32_t num_samples, float prune_threshold,
                                        const float *priority, uint8_t *keep, uint32_t *family);
cuking_status cuking_unrelated_set(cuking_ctx *ctx, const cuking_result *d_records,
                                   uint64_t num_records, uint32_t num_samples,
                                   float prune_threshold, const float *d_priority,
                                   uint8_t *d_keep, uint32_t *d_family, uint32_t *rounds,
                                   void *stream);

/* Site QC: genotype counts per site and per sample, a site mask from the usual rule, and the
 * bitset compacted to the kept sites -- the step between a loaded cohort (a .bed arrives
 * unfiltered) and everything that reads a bitset, which then runs unchanged on a smaller
 * words_per_sample.
 *
 * Layout (cuking.cu:507-523): uint64 bits[num_stored][words_per_sample], P = words_per_sample
 * / 2 plane words, each sample [het words | hom_var words], site s = bit s & 63 of word s >> 6;
 * (het, hom_var) = 00 hom-ref, 10 het, 01 hom-var, 11 missing; sites from num_sites to 64 P are
 * padding and read as missing.  All calls take a plain range of num_stored rows, not a block:
 * the caller of an off-diagonal block passes its rows and columns as it sees fit.
 *
 * cuking_site_counts: for every plane site 0 .. 64 P - 1, the number of the num_stored samples
 * that are hom-ref, het, hom-var and missing is ADDED to d_counts[site][0 .. 3] (uint32
 * [64 P][4], zeroed by the caller before the first call).  The four counts of a site sum to
 * the number of samples counted; padding sites come out as missing += num_stored.  Because the
 * call accumulates, row ranges, tile ranges and GPUs merge by sum; integer sums only, so the
 * result does not depend on launch shape or timing.  One read of the bitset (king_site_qc.hip).
 * cuking_sample_counts: OVERWRITES d_counts[sample][0 .. 3] (uint32 [num_stored][4]) with the
 * (hom_ref, het, hom_var, missing) of each stored sample over the sites [0, num_sites) only:
 * padding is not counted, the four sum to num_sites.  words_per_sample must be
 * cuking_words_per_sample(num_sites).
 * Both: INVALID_ARGUMENT for a null pointer (with num_stored != 0) and a words_per_sample that
 * is zero or odd; num_stored == 0 returns OK without work.  Asynchronous on `stream`.
 *
 * cuking_site_mask_host, the site rule (host only: O(sites) work on 16 B per site).  With
 * called = hom_ref + het + hom_var, n = called + missing, alt = het + 2 hom_var and minor =
 * min(alt, 2 called - alt), site s is kept iff ALL of
 *     s < num_sites
 *     called > 0
 *     (double)called >= (double)min_call_rate * (double)n
 *     (double)minor  >= (double)min_maf * (double)(2 called)
 *     minor >= min_mac
 *     bit s of `also`, if `also` is not NULL ([P] words, site s = bit s & 63 of word s >> 6)
 * each inequality one IEEE double product and one comparison, nothing fused.  {0, 0, 0} keeps
 * every site with one called genotype; min_maf above 0.5 is legal and keeps nothing.  keep
 * receives [plane_words] words in the same bit order, *num_kept (may be NULL) their popcount.
 * INVALID_ARGUMENT: a null counts / filter / keep pointer; plane_words !=
 * cuking_words_per_sample(num_sites) / 2; a rate or frequency outside [0, 1] or NaN.
 * The compaction takes ANY mask: an LD-pruned site list, an HWE test or a region list is
 * applied by passing its mask (or by passing it here as `also`).
 *
 * cuking_compact_sites_host / cuking_compact_sites: with K = popcount(keep), the k-th kept site
 * (ascending) of every sample becomes site k of the output, in both planes; every bit from K to
 * the end of the output plane is missing (1 in both planes).  The output is, byte for byte, the
 * bitset cuking_pack_host builds from an all-ones one for the genotypes restricted to the kept
 * sites.  keep: [words_per_sample_in / 2] words in HOST memory for both functions; it may be
 * freed when the call returns.  Out of place: the output must not overlap the input.  Every
 * output word is written once with a plain store, nothing else is written: no memset is needed.
 * INVALID_ARGUMENT: K = 0 ("no site passes"); a null pointer; a words_per_sample that is zero
 * or odd; words_per_sample_in != cuking_words_per_sample(num_sites_in); words_per_sample_out !=
 * cuking_words_per_sample(K); a keep bit at or beyond num_sites_in; overlapping buffers.
 * num_stored == 0 returns OK without work (after the checks).
 * cuking_compact_sites derives a table of 64 B per input plane word and 4 B per output plane
 * word from keep and uploads it into the context's per-stream cache, ordered on `stream`; it
 * waits for that upload (and so for what `stream` held before), the kernel itself is
 * asynchronous.  One caller per context at a time, like the compute entry points.
 * Out of scope: the C++ `cuking` binary; several ranks (LD pruning and the Hardy-Weinberg test:
 * below); sample filtering and reordering; in-place compaction; filtering inside the .bed loader
 * before the transpose; rewriting a .bim. */
typedef struct cuking_site_filter {
  float min_call_rate; /* called / (called + missing), in [0, 1] */
  float min_maf;       /* minor / (2 called), in [0, 1] */
  uint32_t min_mac;    /* minor allele count */
} cuking_site_filter;
cuking_status cuking_site_counts(cuking_ctx *ctx, const uint64_t *d_bit_set,
                                 uint32_t num_stored, uint32_t words_per_sample,
                                 uint32_t *d_counts, void *stream);
cuking_status cuking_sample_counts(cuking_ctx *ctx, const uint64_t *d_bit_set,
                                   uint32_t num_stored, uint32_t words_per_sample,
                                   uint32_t num_sites, uint32_t *d_counts, void *stream);
cuking_status cuking_site_mask_host(const uint32_t *counts, uint32_t num_sites,
                                    uint32_t plane_words, const cuking_site_filter *filter,
                                    const uint64_t *also, uint64_t *keep, uint32_t *num_kept);
cuking_status cuking_compact_sites_host(const uint64_t *bit_set_in, uint32_t num_stored,
                                        uint32_t words_per_sample_in, const uint64_t *keep,
                                        uint32_t num_sites_in, uint64_t *bit_set_out,
                                        uint32_t words_per_sample_out);
cuking_status cuking_compact_sites(cuking_ctx *ctx, const uint64_t *d_in, uint32_t num_stored,
                                   uint32_t words_per_sample_in, const uint64_t *keep,
                                   uint32_t num_sites_in, uint64_t *d_out,
                                   uint32_t words_per_sample_out, void *stream);

/* LD pruning: which sites to keep so that no two kept sites within a window of variants are
 * correlated above a threshold -- the thinning every protocol runs between site QC and KING, on
 * the bitset where it lies.  Two calls produce the EDGES (pairs of sites with r^2 above the
 * threshold); cuking_unrelated_set, with sites as its "samples" and the minor allele frequency
 * as the priority, picks the kept set; cuking_compact_sites applies it.  csrc/king_ld.h holds
 * every definition below as code shared by host, device and tests.
 *
 * Site-major bitset: Q = ceil(num_stored / 64); uint64 site_bits[num_sites][2][Q], plane 0 =
 * het, plane 1 = hom_var, sample s = bit s % 64 of word s / 64, missing = both bits, bits of
 * samples >= num_stored in the last word SET in both planes (the tail reads as missing).  Only
 * the num_sites real sites have rows; the padding sites of the input are not transposed.
 * cuking_transpose_sites_host / cuking_transpose_sites: the bit transpose of the sample-major
 * bitset [num_stored][words_per_sample] into that form.  Every output word is written once with
 * a plain store: no memset is needed.  INVALID_ARGUMENT: a null pointer; words_per_sample !=
 * cuking_words_per_sample(num_sites); words_per_site_plane != Q; num_stored > 2^24.  num_sites
 * == 0 or num_stored == 0 returns OK without work (after the checks).  Asynchronous on `stream`.
 *
 * Per-pair sums, for sites a < b, with N = ~(het & hom) (called), H = het & ~hom, V = hom &
 * ~het per site, the dosage g = H + 2 V and pc the popcount over all Q words:
 *     n = pc(Na & Nb)
 *     Sx = pc(Ha & Nb) + 2 pc(Va & Nb),  Sxx = pc(Ha & Nb) + 4 pc(Va & Nb); Sy, Syy likewise
 *     Sxy = pc(Ha & Hb) + 2 pc(Ha & Vb) + 2 pc(Va & Hb) + 4 pc(Va & Vb)
 *     cov = n Sxy - Sx Sy,  vx = n Sxx - Sx^2,  vy = n Syy - Sy^2     (int64)
 * num_stored <= 2^24 makes each an integer below 2^53: it converts to double exactly.
 * Edge rule: (a, b) is an edge iff ALL of
 *     a < b < num_sites
 *     b - a < window                       (a window of W variants: pairs up to W - 1 apart)
 *     group[a] == group[b]                 (when group is not NULL: chromosomes)
 *     vx > 0 and vy > 0
 *     (double)cov * (double)cov > ((double)r2_threshold * (double)vx) * (double)vy
 * -- three IEEE double products, each rounded once, no addition, nothing fused: host and device
 * agree bit for bit.  A monomorphic or all-missing site has no edges; r2_threshold = 1 yields no
 * edge at all (for perfectly correlated sites both sides round the same integer).
 * Edge record: cuking_result {sample_i = a, sample_j = b, kin = (float)((double)cov *
 * (double)cov / ((double)vx * (double)vy)), ibs0 = n, ibs1 = ibs2 = 0}.  Record order is
 * unspecified; the set is the contract.
 *
 * cuking_ld_edges_host / cuking_ld_edges: EVERY edge is counted, those whose slot is below
 * max_records are stored; *num_records (HOST memory) receives the exact count.  A count above
 * 2^30 (what cuking_unrelated_set accepts) returns INVALID_ARGUMENT; otherwise a count above
 * max_records returns CUKING_ERR_RESOURCE_EXHAUSTED -- nothing is written past the buffer, the
 * caller retries once with exactly *num_records.  cuking_ld_edges WAITS for `stream` (it reads
 * the count back).  INVALID_ARGUMENT before any work: a null site_bits / num_records pointer, a
 * null records pointer with max_records != 0; num_stored > 2^24; window < 2; r2_threshold NaN
 * or outside [0, 1].  num_sites < 2 or num_stored == 0 gives 0 edges.
 *
 * Default priority of a site from its cuking_site_counts row, with called, alt and minor as in
 * cuking_site_mask_host: cuking_ld_priority = (float)((double)minor / (double)(2 called)), NaN
 * when called == 0 (ranked last by cuking_unrelated_key); among equals the lower site wins.
 * Kept set: cuking_unrelated_set(edges, prune_threshold = -inf, priority).  No two kept sites
 * of one group within the window have r^2 above the threshold, and every dropped site has a
 * kept neighbour.  It keeps the higher-MAF site of a correlated pair, as PLINK does, but it is
 * deliberately NOT PLINK's sliding, order-dependent removal: it has one well-defined answer.
 * Out of scope: the C++ `cuking` binary and several ranks; windows in base pairs; PLINK's
 * step-wise removal order; reading the site-major form straight from a .bed; a VIF-based
 * --indep; phased or haplotype r^2; rewriting a .bim. */
uint32_t cuking_ld_site_words(uint32_t num_stored); /* Q */
float cuking_ld_priority(const uint32_t counts[4]);
cuking_status cuking_transpose_sites_host(const uint64_t *bit_set, uint32_t num_stored,
                                          uint32_t words_per_sample, uint32_t num_sites,
                                          uint64_t *site_bits, uint32_t words_per_site_plane);
cuking_status cuking_transpose_sites(cuking_ctx *ctx, const uint64_t *d_bit_set,
                                     uint32_t num_stored, uint32_t words_per_sample,
                                     uint32_t num_sites, uint64_t *d_site_bits,
                                     uint32_t words_per_site_plane, void *stream);
cuking_status cuking_ld_edges_host(const uint64_t *site_bits, uint32_t num_sites,
                                   uint32_t num_stored, uint32_t window, float r2_threshold,
                                   const int32_t *group, cuking_result *records,
                                   uint64_t max_records, uint64_t *num_records);
cuking_status cuking_ld_edges(cuking_ctx *ctx, const uint64_t *d_site_bits, uint32_t num_sites,
                              uint32_t num_stored, uint32_t window, float r2_threshold,
                              const int32_t *d_group, cuking_result *d_records,
                              uint64_t max_records, uint64_t *num_records, void *stream);

/* Genotype matrix products: the 2-bit genotype matrix times a dense float32 matrix, without
 * ever expanding the genotypes -- what randomized PCA (cuking_amd/pca.py), projection and
 * association scans need from the big data.  csrc/king_geno.h holds the decode as code shared
 * by host, device and tests.
 *
 *     bits   uint64 [num_rows][words_per_row]; words_per_row even, W = words_per_row / 2; a row
 *            is [W het words | W hom_var words]; column k = bit k & 63 of word k >> 6;
 *            num_cols <= 64 W
 *     code(r,k)  0 hom-ref (00), 1 het (het bit only), 2 hom-var (hom_var bit only), 3 missing
 *            (both bits) -- the order of cuking_site_counts
 *     table  float32 [num_cols][4] with CUKING_GENO_TABLE_PER_COLUMN,
 *            float32 [num_rows][4] with CUKING_GENO_TABLE_PER_ROW
 *     B      float32 [num_cols][ldb]
 *     out    float32 [num_rows][ldo]; 1 <= num_rhs <= CUKING_GENO_RHS_MAX; ldb, ldo >= num_rhs
 *     out[r][c] = sum over k < num_cols of table(r or k)[code(r,k)] * B[k][c],  c < num_rhs
 *
 * Both bitsets fit with no conversion: the sample-major one with num_cols = num_sites and a
 * per-column table (Z B), and the site-major planes of cuking_transpose_sites with
 * words_per_row = 2 Q, num_cols = num_stored and a per-row table (Z^T A; the tail bits there
 * read as missing).  Columns at or beyond num_cols contribute nothing, whatever their bits
 * hold.  out[r][0 .. num_rhs) is OVERWRITTEN with plain stores; the elements between num_rhs
 * and ldo are left alone.  cuking_geno_matmul is asynchronous on `stream`.
 *
 * Numerics (inputs finite): the result differs from the real-number sum by at most
 * (num_cols + 2) 2^-24 sum_k |table B| -- the bound of a float32 accumulation of num_cols terms
 * in any order with one rounding per product and per addition.  The device adds in ascending k
 * with one fused multiply-add per term (the f32-input MFMA of gfx950); the host twin accumulates
 * in double and rounds once.  So when every table entry and every B entry is an integer and
 * sum_k |table B| < 2^24, the result is EXACT, on both.  The same inputs give the same bits on
 * every call, stream and launch: one workgroup owns an output row over the whole k range, there
 * are no atomics, no partial sums and no split of k.
 *
 * INVALID_ARGUMENT before any device is touched: words_per_row zero or odd; num_cols > 64 W;
 * num_rhs 0 or above CUKING_GENO_RHS_MAX; ldb or ldo below num_rhs; an unknown table axis; and,
 * with work to do, a null pointer (out when num_rows != 0; bits, table, B when num_cols != 0 as
 * well).  num_rows == 0 returns OK without work; num_cols == 0 writes zeros.
 * Out of scope: the C++ `cuking` binary; several ranks; the N x N relationship matrix;
 * half-precision operands; a row gather as part of the call. */
#define CUKING_GENO_RHS_MAX 64
#define CUKING_GENO_TABLE_PER_COLUMN 0
#define CUKING_GENO_TABLE_PER_ROW 1
cuking_status cuking_geno_matmul_host(const uint64_t *bits, uint32_t num_rows,
                                      uint32_t words_per_row, uint32_t num_cols,
                                      const float *table, int table_axis, const float *b,
                                      uint32_t ldb, uint32_t num_rhs, float *out, uint32_t ldo);
cuking_status cuking_geno_matmul(cuking_ctx *ctx, const uint64_t *d_bits, uint32_t num_rows,
                                 uint32_t words_per_row, uint32_t num_cols, const float *d_table,
                                 int table_axis, const float *d_b, uint32_t ldb, uint32_t num_rhs,
                                 float *d_out, uint32_t ldo, void *stream);

/* PC-Relate: the ancestry-adjusted kinship of every pair of a block, from the 2-bit genotypes
 * and a low-rank model of each sample's allele frequencies (Conomos et al. 2016; GENESIS
 * pcrelate, hl.pc_relate) -- what follows principal components fitted on the unrelated set
 * (cuking_amd/pca.py) in PC-AiR / PC-Relate.  KING-robust reads ancestry distance as negative
 * kinship; this estimator does not.  csrc/king_pcrelate.h holds the element functions as code
 * shared by host, device and tests; cuking_amd/pcrelate.py fits beta with the genotype matrix
 * product above.
 *
 *     bits   uint64 [num_stored][words_per_sample], the sample-major bitset, codes as above
 *     X      float32 [num_stored][ldx], d columns used, 1 <= d <= CUKING_PCRELATE_COLUMNS_MAX;
 *            column 0 is the intercept, the others principal-component scores
 *     beta   float32 [num_sites][ldbeta], d columns used
 *     lo, hi float32, 0 <= lo < hi <= 1 (the wrapper passes min_maf and 1 - min_maf)
 *     block  rows [i_begin, i_end) x columns [j_begin, j_end) of the STORED samples (indices
 *            into bits and X), identical ranges or disjoint with rows first
 *     out    float32, out[(i - i_begin) * ldo + (j - j_begin)], ldo in ELEMENTS >= columns
 *
 *     mu(i,s)    = 0.5f * (fmaf chain in ascending c, from 0.0f, of X[i][c] * beta[s][c]): the
 *                  individual-specific allele frequency (zero terms may pad the chain)
 *     valid(i,s) = code(i,s) != 3 and lo < mu < hi (strict float32 comparisons)
 *     r(i,s)     = (float)g - 2.0f * mu when valid, else 0.0f       (g = the code, 0 1 2)
 *     v(i,s)     = sqrtf(mu * (1.0f - mu)) when valid, else 0.0f    (correctly rounded)
 *     num(i,j)   = sum over s < num_sites of r(i,s) r(j,s)
 *     den(i,j)   = sum over s < num_sites of v(i,s) v(j,s)
 *     kin(i,j)   = num / (4.0f * den)                               (IEEE float32 division)
 *
 * No multiply and add of r or v is contracted, so host and device hold the same r and v bit
 * for bit.  The zeros of the invalid elements are what restricts both sums to the jointly valid
 * sites -- there is no pair-wise mask --, and a pair without one gets NaN.  The diagonal is an
 * entry like any other: 2 kin(i,i) - 1 is the inbreeding estimate.  Sites at or beyond
 * num_sites contribute nothing, whatever their bits hold.
 *
 * Numerics.  The device accumulates each sum in float32 in ascending s with one fused
 * multiply-add per term (the f32-input MFMA of gfx950); there is no split of the site range, no
 * atomics and no partial-sum scratch.  The same inputs give the same bytes on every call and
 * stream, kin(i,j) and kin(j,i) are the same bytes, and an entry does not depend on the block
 * it was computed in.  The host twin accumulates both sums in double, rounds each once and
 * divides in float32.  Both stay within (num_sites + 2) 2^-24 sum |r r| and sum |v v| of the
 * sums of their r and v.
 *
 * Every entry of the block is OVERWRITTEN with plain stores (a diagonal block computes both
 * triangles); nothing between the block's columns and ldo is written.  cuking_pcrelate_matrix
 * is asynchronous on `stream`.  INVALID_ARGUMENT before any device is touched: d 0 or above
 * the maximum; ldx or ldbeta below d; num_sites > 64 (words_per_sample / 2); words_per_sample
 * zero or odd; bounds not 0 <= lo < hi <= 1; a null, reversed or overlapping block or one
 * outside num_stored; ldo below the block's columns; and, with work to do, a null pointer (out;
 * bits, X, beta when num_sites != 0 as well).  An empty block returns OK without work;
 * num_sites == 0 writes NaN.
 * Out of scope: the C++ `cuking` binary; several ranks; half-precision operands; a triangular
 * launch for diagonal blocks; GENESIS's "truncate" bound and its kinship rescaling.  (The
 * pairs above a threshold without a matrix, the IBD-sharing k0 / k2 and re-scoring only listed
 * pairs: the sections below.) */
#define CUKING_PCRELATE_COLUMNS_MAX 32
cuking_status cuking_pcrelate_matrix_host(const uint64_t *bits, uint32_t num_stored,
                                          uint32_t words_per_sample, uint32_t num_sites,
                                          const float *x, uint32_t ldx, const float *beta,
                                          uint32_t ldbeta, uint32_t d, float lo, float hi,
                                          const cuking_submatrix *block, float *out,
                                          uint64_t ldo);
cuking_status cuking_pcrelate_matrix(cuking_ctx *ctx, const uint64_t *d_bits, uint32_t num_stored,
                                     uint32_t words_per_sample, uint32_t num_sites,
                                     const float *d_x, uint32_t ldx, const float *d_beta,
                                     uint32_t ldbeta, uint32_t d, float lo, float hi,
                                     const cuking_submatrix *block, float *d_out, uint64_t ldo,
                                     void *stream);

/* PC-Relate records: the pairs of a block whose ancestry-adjusted kinship is above a threshold,
 * as cuking_result records and without a matrix -- the PC-Relate counterpart of
 * cuking_compute_king (hl.pc_relate(min_kinship=...), GENESIS pcrelate followed by a filter).
 * Memory is proportional to the number of relatives, and a list drawn here holds the
 * cross-ancestry relatives a KING threshold misses.  The records are what cuking_unrelated_set
 * and cuking_pcrelate_pairs (stride 24) take.
 *
 *     bits, num_stored, words_per_sample, num_sites, X, ldx, beta, ldbeta, d, lo, hi, block
 *                 exactly as cuking_pcrelate_matrix takes them
 *     min_kin     float32 threshold, not NaN (-inf and +inf are allowed)
 *     records     room for max_records cuking_result; may be null when max_records == 0
 *     num_records HOST memory: receives the number of qualifying pairs
 *
 * Pairs of a block: a diagonal block (identical ranges) has the entries with i < j, an
 * off-diagonal block (disjoint ranges, rows first) every entry; the diagonal is never a record.
 * A pair is a record iff kin(i, j) > min_kin, the strict float32 comparison a KING record
 * makes, kin being pcrelate_kin(num, den) of the section above from the same r, v and chains.
 * The comparison is false for a NaN: a pair without a jointly valid site is never a record, not
 * even at min_kin = -inf.  A record is {sample_i = i, sample_j = j, kin, ibs0 = ibs1 = ibs2 = 0}
 * with sample_i < sample_j, i and j indices of the stored samples.
 *
 * Device: kin is the same bytes as the entry cuking_pcrelate_matrix writes for that pair, in
 * any block that holds it; only the upper triangle of a diagonal block's tiles is launched
 * (csrc/king_pcrelate.h: pcrelate_triangle_tile).  The ORDER of the records is unspecified and
 * may differ between calls: the set is the contract (sort with cuking_sort_results).  Host
 * twin: kin is the same bytes as cuking_pcrelate_matrix_host, records in ascending (i, j).
 *
 * EVERY qualifying pair is counted, those whose slot is below max_records are stored, and
 * *num_records receives the exact count (it starts at zero on every call).  A count above
 * max_records returns RESOURCE_EXHAUSTED with nothing written past the buffer -- which of the
 * records were stored is then unspecified on the device, the first max_records on the host --
 * and the caller retries with exactly *num_records; max_records == 0 with null records is the
 * counting call.  There is no 2^30 limit here; cuking_unrelated_set has its own.
 * cuking_pcrelate_records WAITS for `stream` (it reads the count back).
 *
 * INVALID_ARGUMENT before any device is touched: everything cuking_pcrelate_matrix refuses
 * about the model and the block, through the same check; a NaN min_kin; a null num_records; a
 * null records with max_records != 0; and, with work to do, a null bits, X or beta.  An empty
 * block, a 1 x 1 diagonal block and num_sites == 0 give 0 records and OK.
 *
 * cuking_pcrelate_triangle_tiles / _index / _tile expose the tile map of a diagonal block for
 * tests: side x side tiles, the tiles tile_j >= tile_i numbered row by row; side at most
 * CUKING_PCRELATE_TRIANGLE_SIDE_MAX.  _tiles returns 0, _index UINT64_MAX and _tile 0 for
 * arguments outside the map.
 * Out of scope: the C++ `cuking` binary; several ranks; a triangular MATRIX call; IBS counts in
 * the record; k0 / k2 inside the scan (cuking_pcrelate_pairs on the records gives them). */
#define CUKING_PCRELATE_TRIANGLE_SIDE_MAX (1ull << 25)
cuking_status cuking_pcrelate_records_host(const uint64_t *bits, uint32_t num_stored,
                                           uint32_t words_per_sample, uint32_t num_sites,
                                           const float *x, uint32_t ldx, const float *beta,
                                           uint32_t ldbeta, uint32_t d, float lo, float hi,
                                           const cuking_submatrix *block, float min_kin,
                                           cuking_result *records, uint64_t max_records,
                                           uint64_t *num_records);
cuking_status cuking_pcrelate_records(cuking_ctx *ctx, const uint64_t *d_bits,
                                      uint32_t num_stored, uint32_t words_per_sample,
                                      uint32_t num_sites, const float *d_x, uint32_t ldx,
                                      const float *d_beta, uint32_t ldbeta, uint32_t d, float lo,
                                      float hi, const cuking_submatrix *block, float min_kin,
                                      cuking_result *d_records, uint64_t max_records,
                                      uint64_t *num_records, void *stream);
uint64_t cuking_pcrelate_triangle_tiles(uint64_t side);
uint64_t cuking_pcrelate_triangle_index(uint64_t side, uint32_t tile_i, uint32_t tile_j);
uint32_t cuking_pcrelate_triangle_tile(uint64_t side, uint64_t index, uint32_t *tile_i,
                                       uint32_t *tile_j);

/* PC-Relate for listed pairs: kinship and the IBD-sharing coefficients k0, k1, k2 of a LIST of
 * pairs -- typically the records of cuking_compute_king -- without a matrix (the estimators of
 * Conomos et al. 2016 as hl.pc_relate states them).  csrc/king_pcrelate.h holds the element
 * functions and the per-site update as code shared by host, device and tests.
 *
 *     bits, X, beta, d, lo, hi   exactly as cuking_pcrelate_matrix takes them
 *     f       float32 [num_stored], the samples' inbreeding coefficients, or null (all 0.0f)
 *     pairs   num_pairs entries, entry p read as two uint32 (i, j) at pairs + p * pair_stride
 *             BYTES; pair_stride >= 8 and a multiple of 4, pairs 4-byte aligned: a cuking_result
 *             buffer (stride 24) or a plain [P][2] array (stride 8).  i and j index the stored
 *             samples in any order; i == j (the self pair) and repeats are allowed
 *     out     one cuking_pcrelate_pair per entry, in input order, written with plain stores
 *
 * Per element, on top of mu, valid, r and v above (no multiply and add contracted):
 *     var = mu * (1.0f - mu)              (the product v takes the root of)
 *     s2  = (1.0f + f_i) * var            when valid, else 0.0f
 *     dom = mu, 0.0f, 1.0f - mu           for the codes 0, 1, 2
 *     e   = dom - s2                      when valid, else 0.0f
 * Per pair, over the JOINTLY valid sites s < num_sites (both elements valid; any other site
 * adds nothing), each float sum ONE float32 chain from +0.0f in ascending s, one fmaf per term:
 *     num   fmaf(r_i, r_j, .)      den   fmaf(v_i, v_j, .)
 *     dnum  fmaf(e_i, e_j, .)      dden  fmaf(s2_i, s2_j, .)
 *     hden  fmaf(a, a, .) then fmaf(b, b, .), a = mu_i * (1.0f - mu_j), b = (1.0f - mu_i) * mu_j
 *     ibs0  uint32: the sites with codes (0, 2) or (2, 0);  sites  uint32: all of them
 * In these chains i is the SMALLER index of the entry and j the larger (the order matters to
 * hden's rounding only), which is what makes (i, j) and (j, i) the same bytes; sample_i and
 * sample_j of the output row are copied from the input as they stand.  Then, in IEEE float32:
 *     kin = num / (4.0f * den)            k2 = dnum / dden
 *     k0  = kin > CUKING_PCRELATE_K0_SWITCH ? (1.0f - 4.0f * kin) + k2 : (float)ibs0 / hden
 *           (the comparison is false for a NaN)
 *     k1  = (1.0f - k2) - k0
 * A NaN is stored as the quiet NaN 0x7FC00000.  A pair without a jointly valid site gets four
 * NaNs and two zeros; so does a pair with an index >= num_stored, for which no memory outside
 * the arrays is read.  num_sites == 0 writes such rows for every pair.
 *
 * The host twin evaluates the very same chains: host and device agree BIT FOR BIT in every
 * field.  A row depends on its own pair only -- not on its position in the list, the length of
 * the list, the stride, the stream or the call.  One thread runs all sites of a pair, so a
 * short list is bound by that thread's latency, not by throughput.
 *
 * cuking_pcrelate_pairs is asynchronous on `stream`.  INVALID_ARGUMENT before any device is
 * touched: d 0 or above the maximum; ldx or ldbeta below d; num_sites > 64 (words_per_sample /
 * 2); words_per_sample zero or odd; bounds not 0 <= lo < hi <= 1; pair_stride below 8 or not a
 * multiple of 4; and, with work to do, a null pointer (pairs, out; bits, X, beta when
 * num_sites != 0 as well).  num_pairs == 0 returns OK without work.
 * Out of scope: the C++ `cuking` binary; several ranks; GENESIS's rescaling of the
 * coefficients; a k0 / k2 matrix. */
#define CUKING_PCRELATE_K0_SWITCH 0.17677669529663689f /* 2^(-5/2) in float32 */
typedef struct cuking_pcrelate_pair {
  uint32_t sample_i, sample_j; /* copied from the input */
  float kin, k0, k1, k2;
  uint32_t ibs0, sites; /* counts over the jointly valid sites */
} cuking_pcrelate_pair;
cuking_status cuking_pcrelate_pairs_host(const uint64_t *bits, uint32_t num_stored,
                                         uint32_t words_per_sample, uint32_t num_sites,
                                         const float *x, uint32_t ldx, const float *beta,
                                         uint32_t ldbeta, uint32_t d, float lo, float hi,
                                         const float *f, const void *pairs, uint64_t num_pairs,
                                         uint32_t pair_stride, cuking_pcrelate_pair *out);
cuking_status cuking_pcrelate_pairs(cuking_ctx *ctx, const uint64_t *d_bits, uint32_t num_stored,
                                    uint32_t words_per_sample, uint32_t num_sites,
                                    const float *d_x, uint32_t ldx, const float *d_beta,
                                    uint32_t ldbeta, uint32_t d, float lo, float hi,
                                    const float *d_f, const void *d_pairs, uint64_t num_pairs,
                                    uint32_t pair_stride, cuking_pcrelate_pair *d_out,
                                    void *stream);

/* IBD segments for listed pairs: the long stretches of the genome in which two samples never
 * carry opposite homozygotes (IBD1) or never differ (IBD2), for a LIST of pairs -- typically the
 * records of cuking_compute_king (KING --ibdseg, IBIS and TRUFFLE do this on unphased data).
 * From their lengths follow the shared proportions, a kinship and the parent-child / full-sibling
 * split with no allele frequency, no principal component and no min_maf.  Everything is decided
 * on integers: host, device and a restatement in numpy agree bit for bit.  csrc/king_ibd.h holds
 * the word masks and the segment test as code shared by host, device and tests.
 *
 *     bits    uint64 [num_stored][words_per_sample], the sample-major bitset; codes as in
 *             cuking_site_counts: 0 hom-ref, 1 het, 2 hom-var, 3 missing
 *     group   int32 [num_sites] or null (one group); sites s - 1 and s are in one group iff the
 *             values are equal (chromosomes, as cuking_ld_edges takes them)
 *     pos     uint32 [num_sites] or null (pos[s] = s); non-decreasing inside a group: base
 *             pairs, or centimorgans as integer micro-Morgans
 *     pairs, num_pairs, pair_stride   exactly as cuking_pcrelate_pairs reads them
 *     out     one cuking_ibd_pair per entry, in input order, written with plain stores
 *
 * For a pair (i, j) and a site s < num_sites:
 *     opp(s)   the codes are (0, 2) or (2, 0)
 *     diff(s)  both are called and the codes differ (opp is a subset of diff)
 * A site that either sample misses is neither.  Bits from num_sites to the end of the plane are
 * never looked at, whatever they hold.
 *     run of kind 1   a maximal interval [a, b] of sites of one group without an opp site
 *     run of kind 2   a maximal interval [a, b] of sites of one group without a diff site
 *     segment         a run with b - a + 1 >= min_sites and pos[b] - pos[a] >= min_length; its
 *                     length is pos[b] - pos[a]
 * A break site belongs to no run; a group boundary ends a run without removing a site; missing
 * sites neither break nor end a run.  Every kind-2 segment lies inside a kind-1 segment, so
 * length2 <= length1.
 *
 * min_sites >= CUKING_IBD_MIN_SITES = 64 is part of the contract: a run of 64 or more sites
 * always closes in a later 64-site word than it starts in, so the runs of up to 63 sites that
 * open and close inside one word can never qualify and the kernel never enumerates bits.  The
 * defaults of the wrappers, min_sites = 512 and min_length = 0, are conventions.
 *
 * (i, j) and (j, i) give the same counts and lengths; sample_i and sample_j are copied from the
 * input as they stand.  The self pair is legal: it has no break, so every group that satisfies
 * the minimum is one segment of both kinds.  A pair with an index >= num_stored gets zeros, and
 * no memory outside the arrays is read for it.  A row depends on its own pair only -- not on its
 * position in the list, the length of the list, the stride, the stream or the call.
 *
 * Segment list (optional).  num_segments null: segments are not enumerated, segments must be
 * null and max_segments 0, and cuking_ibd_pairs is asynchronous on `stream`.  num_segments not
 * null (HOST memory): EVERY segment of every pair is counted, those whose slot is below
 * max_segments are stored as cuking_ibd_segment {pair = the index into the list, kind, first_site
 * = a, last_site = b}, and *num_segments receives the exact count (it starts at zero on every
 * call).  The order is unspecified on the device (the set is the contract) and by (pair, word of
 * the last site's successor, kind) on the host.  A count above max_segments returns
 * RESOURCE_EXHAUSTED with nothing written past the buffer and every row of `out` written; the
 * caller retries with exactly *num_segments; max_segments == 0 with null segments is the
 * counting call.  cuking_ibd_pairs then WAITS for `stream` (it reads the count back); it also
 * waits when pos is given, for the check below.
 *
 * INVALID_ARGUMENT before any device is touched: words_per_sample zero or odd; num_sites > 64
 * (words_per_sample / 2); min_sites < 64; pair_stride below 8 or not a multiple of 4; a segment
 * buffer or a max_segments without num_segments; a segment list for more than 2^32 pairs; and,
 * with work to do, a null pointer (pairs, out; segments when max_segments != 0; bits when
 * num_sites != 0 as well).  FAILED_PRECONDITION before the launch, naming the first offending
 * site: pos[s] < pos[s - 1] inside a group (the device call copies group and pos to the host for
 * this check).  num_pairs == 0 returns OK without work (after the checks of the arguments);
 * num_sites == 0 writes zero rows.
 * One wrong homozygote splits a run; cuking_ibd_pairs_bridged below forgives isolated ones.
 * All pairs of a block, without a list: cuking_ibd_scan ("IBD scan of a block" below).
 * Out of scope: the C++ `cuking` binary; several ranks; phased IBD; recombination maps beyond an
 * integer pos. */
#define CUKING_IBD_MIN_SITES 64
typedef struct cuking_ibd_pair {
  uint32_t sample_i, sample_j;   /* copied from the input */
  uint32_t segments1, segments2; /* number of segments of kind 1 / 2 */
  uint64_t length1, length2;     /* sum of their lengths */
  uint32_t longest1, longest2;   /* largest single length, 0 without a segment */
} cuking_ibd_pair;               /* 40 bytes */
typedef struct cuking_ibd_segment {
  uint32_t pair, kind, first_site, last_site;
} cuking_ibd_segment; /* 16 bytes */
cuking_status cuking_ibd_pairs_host(const uint64_t *bits, uint32_t num_stored,
                                    uint32_t words_per_sample, uint32_t num_sites,
                                    const int32_t *group, const uint32_t *pos,
                                    uint32_t min_sites, uint32_t min_length, const void *pairs,
                                    uint64_t num_pairs, uint32_t pair_stride,
                                    cuking_ibd_pair *out, cuking_ibd_segment *segments,
                                    uint64_t max_segments, uint64_t *num_segments);
cuking_status cuking_ibd_pairs(cuking_ctx *ctx, const uint64_t *d_bits, uint32_t num_stored,
                               uint32_t words_per_sample, uint32_t num_sites,
                               const int32_t *d_group, const uint32_t *d_pos, uint32_t min_sites,
                               uint32_t min_length, const void *d_pairs, uint64_t num_pairs,
                               uint32_t pair_stride, cuking_ibd_pair *d_out,
                               cuking_ibd_segment *d_segments, uint64_t max_segments,
                               uint64_t *num_segments, void *stream);

/* IBD scan of a block: the pairs of a block that share a kind-1 segment, found without a list.
 * The list of "IBD segments for listed pairs" usually is the record buffer of cuking_compute_king
 * or cuking_pcrelate_records, cut at a threshold on the very average the segments improve on: a
 * fourth-degree pair with two long shared stretches and a KING kinship of 0.02 never reaches it.
 * This call looks at every pair, as KING --ibdseg and IBIS do, and keeps the pairs that have
 * something: it is to cuking_ibd_pairs what cuking_pcrelate_records is to the PC-Relate matrix.
 *
 *     bits, num_stored, words_per_sample, num_sites, group, pos, min_sites, min_length
 *                 exactly as cuking_ibd_pairs takes them; runs, segments and lengths are those
 *                 of that section and are strict (no bridging); min_sites >= CUKING_IBD_MIN_SITES
 *     block       exactly as cuking_pcrelate_records takes it: rows x columns of STORED samples
 *     min_total   uint64 threshold on length1; 0 keeps every pair with a segment
 *     records     room for max_records cuking_ibd_pair; may be null when max_records == 0
 *     num_records HOST memory: receives the number of qualifying pairs
 *
 * Pairs of a block: a diagonal block (identical ranges) has the pairs i < j, an off-diagonal
 * block (disjoint ranges, rows first) every pair; the self pair is never a record.
 * Pair (i, j) is a record iff segments1 >= 1 && length1 >= min_total, length1 being the uint64
 * sum of the lengths of its kind-1 segments.  The record is the cuking_ibd_pair with sample_i = i
 * < sample_j = j and, from segments1 on, the same bytes cuking_ibd_pairs[_host] writes for that
 * pair.  The scan decides nothing of its own: it uses the masks, ibd_starts / ibd_closes /
 * ibd_open_start / ibd_close_last and ibd_is_segment of csrc/king_ibd.h.  A record does not
 * depend on the block that holds the pair, on the launch shape, on the stream or on the call.
 *
 * EVERY qualifying pair is counted, those whose slot is below max_records are stored, and
 * *num_records receives the exact count (it starts at zero on every call).  A count above
 * max_records returns RESOURCE_EXHAUSTED with nothing written past the buffer -- which of the
 * records were stored is then unspecified on the device, the first max_records on the host --
 * and the caller retries with exactly *num_records; max_records == 0 with null records is the
 * counting call.  The ORDER of the records is unspecified on the device and may differ between
 * calls: the set is the contract.  Host twin: ascending (i, j).  cuking_ibd_scan WAITS for
 * `stream` once, to read the count back; like cuking_ibd_pairs it waits once more, before the
 * launch, when pos is given (the check below).
 *
 * INVALID_ARGUMENT before any device is touched: a null, reversed or overlapping block, through
 * the check of cuking_pcrelate_records; everything cuking_ibd_pairs refuses about
 * words_per_sample, num_sites and min_sites, through its check; a block outside the stored
 * samples; a null num_records; a null records with max_records != 0; and, with work to do, a
 * null bits.  FAILED_PRECONDITION for a pos that decreases inside a group, through the check of
 * cuking_ibd_pairs.  An empty block, a 1 x 1 diagonal block and num_sites == 0 give 0 records
 * and OK.
 *
 * A screen for the bridged call.  Every run of a chain that cuking_ibd_pairs_bridged links has at
 * least bridge_sites sites, and an unlinked segment has at least min_sites >= bridge_sites sites.
 * So for B >= 64 a scan at min_sites = B, min_length = 0, min_total = 0 records EVERY pair for
 * which the bridged call reports a kind-1 segment, for any bridge_sites = B, any min_sites >= B
 * and any min_length: scan loosely, then give the records' pairs to the bridged call.
 *
 * Device: one workgroup per 32 x 32 tile of pairs, the samples' words staged through LDS once per
 * tile, only the tiles tile_j >= tile_i of a diagonal block (csrc/king_ibd_scan.hip).  Memory is
 * the record buffer, one counter and the group mask: nothing proportional to the pairs.
 * Out of scope: bridging inside the scan; a segment list from the scan (cuking_ibd_pairs with a
 * segment list on the records gives it); the C++ `cuking` binary; several ranks; a threshold on
 * kind 2. */
cuking_status cuking_ibd_scan_host(const uint64_t *bits, uint32_t num_stored,
                                   uint32_t words_per_sample, uint32_t num_sites,
                                   const int32_t *group, const uint32_t *pos, uint32_t min_sites,
                                   uint32_t min_length, const cuking_submatrix *block,
                                   uint64_t min_total, cuking_ibd_pair *records,
                                   uint64_t max_records, uint64_t *num_records);
cuking_status cuking_ibd_scan(cuking_ctx *ctx, const uint64_t *d_bits, uint32_t num_stored,
                              uint32_t words_per_sample, uint32_t num_sites,
                              const int32_t *d_group, const uint32_t *d_pos, uint32_t min_sites,
                              uint32_t min_length, const cuking_submatrix *block,
                              uint64_t min_total, cuking_ibd_pair *d_records,
                              uint64_t max_records, uint64_t *num_records, void *stream);

/* IBD segments with bridged breaks: the call above, tolerant of sparse genotyping errors.  On
 * real calls with 0.1 - 1 % discordance a single wrong homozygote cuts a true IBD stretch into
 * pieces that fall below min_sites; KING --ibdseg, IBIS and TRUFFLE all forgive such errors.
 * Everything of "IBD segments for listed pairs" stays -- codes, opp, diff, groups, pos, runs,
 * missing sites, the segment test -- and one argument is added: bridge_sites, either 0 or >=
 * CUKING_IBD_MIN_SITES.  Still decided on integers and a function of the pair's genotypes only.
 *
 * For one pair and one kind, the runs in site order:
 *     linked    two consecutive runs [a, b] and [a', b'] are linked iff
 *                 a' == b + 2 (exactly one site lies between them: a break of this kind),
 *                 sites b, b + 1, b + 2 lie in one group (no group starts at b + 1 or b + 2),
 *                 b - a + 1 >= bridge_sites and b' - a' + 1 >= bridge_sites (missing sites
 *                 count as sites, as they do for min_sites)
 *     chain     a maximal sequence of runs joined by links; its interval [A, B] goes from the
 *               first site of its first run to the last site of its last run and includes the
 *               bridged break sites
 *     segment   a chain with B - A + 1 >= min_sites and pos[B] - pos[A] >= min_length; its
 *               length is pos[B] - pos[A]
 * Consequences:
 *   - bridge_sites = 0 links nothing: the call above, byte for byte;
 *   - a link depends on the two runs and the site between them only, so the chains are unique;
 *   - a segment has at most one break per bridge_sites + 1 sites;
 *   - two adjacent break sites are never bridged, nor is a break that is the first or the last
 *     site of a group, nor a break at site 0 or at num_sites - 1;
 *   - a run inside a chain may be shorter than min_sites: 100 + 1 + 100 sites pass min_sites =
 *     150 at bridge_sites = 64;
 *   - kind 2 bridges diff sites, kind 1 opp sites, independently.  A bridged diff site that is
 *     also opp is bridged in kind 1 too (the kind-1 runs around it contain the kind-2 runs), so
 *     every kind-2 chain lies inside a kind-1 chain and length2 <= length1 still holds;
 *   - bridge_sites >= 64 plays the part of min_sites >= 64: both runs of a link close in a later
 *     word than they start in, a bridged break is the only break of its 64-site word, and nobody
 *     enumerates bits.
 *
 * out and segments keep their rows; first_site and last_site are the chain's A and B.
 *     bridged   uint32 [num_pairs][2] or null: the links inside the COUNTED segments of kind 1
 *               and of kind 2 -- the number of forgiven errors, what a user looks at to judge
 *               bridge_sites.  Plain stores; zero for a pair with an index >= num_stored.
 * Every refusal of the call above applies, and 0 < bridge_sites < 64 is INVALID_ARGUMENT.  The
 * segment-list buffer rule, the waits, (i, j) == (j, i) and "a row depends on its own pair only"
 * are unchanged.  The order of the segment list is unspecified on the host and on the device:
 * the set is the contract.  (At bridge_sites = 0 the device runs the kernel of the call above.)
 * Out of scope: gaps of more than one site; per-segment error counts in the list; trimming of
 * segment ends; a model of the error rate. */
cuking_status cuking_ibd_pairs_bridged_host(const uint64_t *bits, uint32_t num_stored,
                                            uint32_t words_per_sample, uint32_t num_sites,
                                            const int32_t *group, const uint32_t *pos,
                                            uint32_t min_sites, uint32_t min_length,
                                            uint32_t bridge_sites, const void *pairs,
                                            uint64_t num_pairs, uint32_t pair_stride,
                                            cuking_ibd_pair *out, uint32_t *bridged,
                                            cuking_ibd_segment *segments, uint64_t max_segments,
                                            uint64_t *num_segments);
cuking_status cuking_ibd_pairs_bridged(cuking_ctx *ctx, const uint64_t *d_bits,
                                       uint32_t num_stored, uint32_t words_per_sample,
                                       uint32_t num_sites, const int32_t *d_group,
                                       const uint32_t *d_pos, uint32_t min_sites,
                                       uint32_t min_length, uint32_t bridge_sites,
                                       const void *d_pairs, uint64_t num_pairs,
                                       uint32_t pair_stride, cuking_ibd_pair *d_out,
                                       uint32_t *d_bridged, cuking_ibd_segment *d_segments,
                                       uint64_t max_segments, uint64_t *num_segments,
                                       void *stream);

/* Runs of homozygosity: the long stretches of the genome in which ONE sample carries no
 * heterozygous call -- the IBD of a sample's own two haplotypes (king --roh, plink --homozyg,
 * bcftools roh).  Their summed length over the genome's length is F_ROH, the inbreeding estimate
 * that needs no allele frequency and no principal component; a whole-chromosome run flags
 * uniparental disomy or a large deletion.  It is "IBD segments for listed pairs" with another
 * break mask and one kind, decided on the same integers by the same code (csrc/king_ibd.h).
 *
 * The codes are those of the bitset:
 *     het bit 0, hom bit 0   hom-ref
 *     het bit 1, hom bit 0   het
 *     het bit 0, hom bit 1   hom-var
 *     het bit 1, hom bit 1   missing
 *     break   for one sample and word, brk = het & ~hom (roh_break): a heterozygous call
 *     in      ibd_valid_mask(num_sites, w) & ~brk, the sites inside some run.  A missing
 *             genotype neither breaks nor ends a run; bits at or beyond num_sites never matter
 *             (all-ones padding gives the same bytes)
 * Everything else is "IBD segments" with this `in`: runs per group (ibd_starts / ibd_closes with
 * the group-start mask), THE segment test ibd_is_segment(a, b, pos[a], pos[b], min_sites,
 * min_length) with the length pos[b] - pos[a], and with bridge_sites != 0 the links of "IBD
 * segments with bridged breaks" (ibd_linked) and maximal chains: one isolated het between two
 * runs of at least bridge_sites sites of one group is forgiven (plink --homozyg-window-het 1).
 * min_sites >= CUKING_IBD_MIN_SITES; bridge_sites is 0 or >= 64; group or pos may be null; pos
 * must not decrease inside a group.  The refusals and their messages are those of
 * cuking_ibd_pairs_bridged (a null list of samples is legal, and there is no stride).
 *
 *     samples   uint32 [num_samples] or null: the samples 0 .. num_samples - 1.  Repeats and any
 *               order are allowed
 *     out       one cuking_roh_sample of 24 bytes per listed sample, in list order, plain stores.
 *               `bridged` counts the bridged het sites inside the counted segments and is 0 at
 *               bridge_sites == 0.  A listed index >= num_stored loads nothing and gets zeros
 *               with `sample` echoed.  A row depends on its own sample only
 * Segment list (optional): cuking_ibd_segment rows with pair = the row index, kind =
 * CUKING_ROH_KIND and first_site / last_site the chain's ends, in no specified order.  The buffer,
 * the count, RESOURCE_EXHAUSTED and the waits are exactly those of cuking_ibd_pairs; without a
 * list (num_segments null) and without pos the call is asynchronous on its stream.
 * Out of scope: a maximum gap between neighbouring sites (pass chromosome arms as `group`);
 * PLINK's sliding-window and density rules; more than one het per bridge; allele-frequency or
 * LOD-weighted runs; several ranks. */
#define CUKING_ROH_KIND 0
typedef struct cuking_roh_sample {
  uint64_t length;                              /* sum of the segments' lengths */
  uint32_t sample, segments, longest, bridged;  /* the listed index; count; largest length */
} cuking_roh_sample;                            /* 24 bytes */
cuking_status cuking_roh_samples_host(const uint64_t *bits, uint32_t num_stored,
                                      uint32_t words_per_sample, uint32_t num_sites,
                                      const int32_t *group, const uint32_t *pos,
                                      uint32_t min_sites, uint32_t min_length,
                                      uint32_t bridge_sites, const uint32_t *samples,
                                      uint64_t num_samples, cuking_roh_sample *out,
                                      cuking_ibd_segment *segments, uint64_t max_segments,
                                      uint64_t *num_segments);
cuking_status cuking_roh_samples(cuking_ctx *ctx, const uint64_t *d_bits, uint32_t num_stored,
                                 uint32_t words_per_sample, uint32_t num_sites,
                                 const int32_t *d_group, const uint32_t *d_pos,
                                 uint32_t min_sites, uint32_t min_length, uint32_t bridge_sites,
                                 const uint32_t *d_samples, uint64_t num_samples,
                                 cuking_roh_sample *d_out, cuking_ibd_segment *d_segments,
                                 uint64_t max_segments, uint64_t *num_segments, void *stream);

/* Mendelian errors: the sites at which a child's genotype cannot come from its parents'
 * (plink --mendel, hl.mendel_errors, the trio check of KING --build and of gnomAD's sample QC),
 * counted per trio or duo and per site on the bitset where it lies.  The counts confirm or reject
 * a declared or inferred trio, point at the sample that is wrong, and name the sites that are.
 * Integers only: host twin and kernel agree byte for byte (csrc/king_mendel.h is the definition as
 * code, mendel_code_masks, used by both and by the tests).
 *
 * Per sample and word, with valid = ibd_valid_mask(num_sites, w) (the codes of the bitset as under
 * "Runs of homozygosity"):
 *     R = ~het & ~hom & valid   hom-ref
 *     H =  het & ~hom & valid   het
 *     V =  hom & ~het & valid   hom-var
 *     C = R | H | V             called
 * A parent that is absent reads as missing everywhere (R = H = V = 0): its index is
 * CUKING_MENDEL_NO_PARENT, or a listed index >= num_stored, which loads nothing.  The error codes
 * carry the numbers of PLINK and Hail, autosomal only (f father, m mother, c child):
 *     code   father   mother   child
 *       1      R        R        H
 *       2      V        V        H
 *       3      V      not V      R
 *       4    not V      V        R
 *       5      V        V        R
 *       6      R      not R      V
 *       7    not R      R        V
 *       8      R        R        V
 * "not V" and "not R" include missing and absent, so a duo with a father can only show codes 3 and
 * 6 and a duo with a mother only 4 and 7.  The eight masks are pairwise disjoint; their OR is the
 * error mask of the trio and word.  Bits at or beyond num_sites never matter (all-ones and
 * all-zero padding give the same bytes).
 *
 * cuking_mendel_trios:
 *     trios       uint32 [num_trios][3]: child, father, mother.  Repeats, any order, shared parents,
 *                 a child that is its own parent are all legal
 *     out         one cuking_mendel_trio of 48 bytes per listed trio, in list order, plain stores:
 *                 the three indices echoed, errors[k] = the number of sites with code k + 1, and
 *                 called = the number of sites where the child and every parent whose index is not
 *                 CUKING_MENDEL_NO_PARENT are called (a listed parent >= num_stored: 0).  A child
 *                 >= num_stored gives zeros.  A row depends on its own three indices only
 *     error_bits  null, or uint64 [num_trios][W], W = words_per_sample / 2: the error mask of
 *                 every trio and word (zero at and beyond num_sites), plain stores
 * Refused with INVALID_ARGUMENT: a null context (device form), words_per_sample zero or odd,
 * num_sites > 64 W, and with num_trios != 0 a null trios, out or (num_sites != 0) bits pointer.
 * num_trios == 0 is no work.  No atomics: the result cannot depend on timing or launch shape.  The
 * device call is asynchronous on its stream, with or without error_bits.
 *
 * cuking_mendel_site_counts ADDS, for every plane site 0 .. 64 W - 1, the number of the num_trios
 * rows of error_bits (uint64 [num_trios][W]) whose bit is set to counts (uint32 [64 W]): like
 * cuking_site_counts it accumulates, so chunks of trios merge by sum.  Refused: a null context, W
 * == 0, num_trios >= 2^32 (a count has 32 bits), and with num_trios != 0 a null pointer.
 * Asynchronous on its stream.
 * Out of scope: X, Y and haploid codes 9-12; setting erroneous genotypes to missing; sex; more
 * than one generation; per-error rows; several ranks. */
#define CUKING_MENDEL_NO_PARENT 0xFFFFFFFFu
typedef struct cuking_mendel_trio {
  uint32_t child, father, mother; /* as listed */
  uint32_t called;                /* sites where everyone who is not NO_PARENT is called */
  uint32_t errors[8];             /* errors[k]: sites with code k + 1 */
} cuking_mendel_trio;             /* 48 bytes */
cuking_status cuking_mendel_trios_host(const uint64_t *bits, uint32_t num_stored,
                                       uint32_t words_per_sample, uint32_t num_sites,
                                       const uint32_t *trios, uint64_t num_trios,
                                       cuking_mendel_trio *out, uint64_t *error_bits);
cuking_status cuking_mendel_trios(cuking_ctx *ctx, const uint64_t *d_bits, uint32_t num_stored,
                                  uint32_t words_per_sample, uint32_t num_sites,
                                  const uint32_t *d_trios, uint64_t num_trios,
                                  cuking_mendel_trio *d_out, uint64_t *d_error_bits,
                                  void *stream);
cuking_status cuking_mendel_site_counts_host(const uint64_t *error_bits, uint64_t num_trios,
                                             uint32_t plane_words, uint32_t *counts);
cuking_status cuking_mendel_site_counts(cuking_ctx *ctx, const uint64_t *d_error_bits,
                                        uint64_t num_trios, uint32_t plane_words,
                                        uint32_t *d_counts, void *stream);

/* Hardy-Weinberg test: the exact test of Wigginton, Cutler and Abecasis (2005) per site from its
 * genotype counts (plink --hwe, hl.hardy_weinberg_test) -- the site-QC rule that needs more than a
 * comparison, computed where the counts lie.  csrc/king_hwe.h holds the definition below as code
 * (hwe_exact_p), shared by kernel, host twin and tests; only *, /, +, - and comparisons on IEEE
 * doubles in ONE order, so host, device and a restatement in any language with doubles agree bit
 * for bit.
 *
 * p(hom_ref, het, hom_var, midp), with n = hom_ref + het + hom_var:
 *     n == 0 gives 1.0; n > 2^24 (the library's sample limit) gives NaN.
 *     r0 = min(hom_ref, hom_var), c0 = max(hom_ref, hom_var); total = 1.0, tail = 1.0: the
 *     observed table is term 1.0 and counts as "no more likely than itself".
 *     Up (more hets): t = 1, x = het, hr = r0, hc = c0, all doubles.  While hr > 0:
 *         t = (t * (4.0 * hr * hc)) / ((x + 2.0) * (x + 1.0));  x += 2; hr -= 1; hc -= 1;
 *         if t == 0.0 the direction ends (every later term is 0);
 *         if !(t < inf) the result is 0.0 (another table is more than 10^308 times as likely);
 *         otherwise total += t, and tail += t if t <= 1 + 2^-27.
 *     Down (fewer hets): again from t = 1, x = het, hr = r0, hc = c0.  While x >= 2:
 *         t = (t * (x * (x - 1.0))) / (4.0 * (hr + 1.0) * (hc + 1.0));  x -= 2; hr += 1; hc += 1;
 *         followed by the same three steps.
 *     if midp: tail -= 0.5 (half the observed table's probability, Graffelman and Moreno 2013).
 *     p = tail / total.
 * Both integer products stay below 2^50 and are exact; up is summed before down; subnormal terms
 * are kept (nothing is flushed to zero).  The tie constant 1 + 2^-27 is derived: a table exactly as
 * likely as the observed one is reached after at most 2^24 steps of two roundings each, so its
 * computed term is within 2 * 2^24 * 2^-53 = 2^-28 of 1 -- every exact tie is counted.
 *
 * cuking_hwe_sites / cuking_hwe_sites_host:
 *     counts   uint32 [.][4], the array of cuking_site_counts: hom_ref, het, hom_var, missing
 *              (ignored); rows [0, num_sites) are read.  Device form: 16-byte aligned
 *     p        double [num_sites], overwritten with plain stores
 *     flags    CUKING_HWE_MIDP or 0
 * Refused with INVALID_ARGUMENT: a null context (device form), any other flag bit, with num_sites
 * != 0 a null pointer, and a misaligned device pointer.  num_sites == 0 is no work.  The device
 * call (king_hwe.hip: one thread per site, one chain per owner) is asynchronous on `stream`; no
 * atomics, no scratch buffer, nothing data-dependent that can fail.  A site is kept by the usual
 * rule iff p >= threshold, which is false for NaN; the mask goes to cuking_site_mask_host as `also`.
 * Out of scope: a lane-parallel split of one site's walk (it would change the rounding order);
 * log-space or lgamma forms; the chi-square test; X-chromosome and haploid HWE; ancestry-adjusted
 * HWE; choosing founder or control rows (the caller counts the rows it wants); excess versus
 * deficit; the C++ `cuking` binary; several ranks. */
#define CUKING_HWE_MIDP 1u
cuking_status cuking_hwe_sites_host(const uint32_t *counts, uint32_t num_sites, uint32_t flags,
                                    double *p);
cuking_status cuking_hwe_sites(cuking_ctx *ctx, const uint32_t *d_counts, uint32_t num_sites,
                               uint32_t flags, double *d_p, void *stream);

/* PI_HAT (PLINK --genome): the method-of-moments IBD estimate of PLINK --genome and
 * hl.identity_by_descent -- Z0, Z1, Z2 and PI_HAT of a pair from its IBS0/1/2 counts and the
 * cohort's allele frequencies -- and a scan of a block that decides on PI_HAT instead of on KING
 * kinship.  csrc/king_pihat.h holds the definition below as code, shared by kernel, host twins
 * and tests; only *, /, +, - and comparisons on IEEE doubles in ONE written order with no
 * contraction, so host, device and a restatement in any language with doubles agree bit for bit.
 *
 * Model, from the count rows of cuking_site_counts (hom_ref = r, het = h, hom_var = v of the rows
 * the frequencies come from: founders, an unrelated set, or the cohort itself): n = r + h + v,
 * x = h + 2 v, y = h + 2 r, N = x + y.  F(a, k) = a (a - 1) ... (a - k + 1), multiplied left to
 * right, 0 as soon as a factor is 0.  A site is used iff n >= 2; its terms are the probabilities
 * of drawing the alleles of two people without replacement (PLINK's finite-sample corrections):
 *     a00 = (2 (F(x,2) F(y,2))) / F(N,4)
 *     a01 = (4 (F(x,3) F(y,1) + F(x,1) F(y,3))) / F(N,4)
 *     a02 = ((F(x,4) + F(y,4)) + 4 (F(x,2) F(y,2))) / F(N,4)
 *     a11 = (2 (F(x,2) F(y,1) + F(x,1) F(y,2))) / F(N,3)
 *     a12 = (((F(x,3) + F(y,3)) + F(x,2) F(y,1)) + F(x,1) F(y,2)) / F(N,3)
 * (a00 + a01 + a02 = 1 and a11 + a12 = 1 in exact arithmetic), and E_uv = (the sum of a_uv over
 * the used sites, in site order) / sites_used.  With no used site the model holds NaNs and no
 * pair qualifies.  A row with more than 2^24 people fails the call.
 *
 * Pair, with S = ibs0 + ibs1 + ibs2 as doubles:
 *     z0 = ibs0 / (e00 S)
 *     z1 = (ibs1 - z0 (e01 S)) / (e11 S)
 *     z2 = ((ibs2 - z0 (e02 S)) - z1 (e12 S)) / S
 * Bounded (the default: PLINK without --nudge, Hail's bounded=True), in this order: z0 > 1 ->
 * (1, 0, 0); z1 > 1 -> (0, 1, 0); z2 > 1 -> (0, 0, 1); z0 < 0 -> z0 = 0 and z1, z2 divided by
 * z1 + z2; z1 < 0 -> z1 = 0 and z0, z2 divided by z0 + z2; z2 < 0 -> z2 = 0 and z0, z1 divided by
 * z0 + z1.  CUKING_PIHAT_UNBOUNDED skips the bounding.  pi_hat = z1 / 2 + z2.  A record's `kin`
 * field holds (float)pi_hat, and a pair qualifies iff (float)pi_hat > min_pi_hat: the strict
 * float32 comparison of every record of this library, false for NaN.  Where this text and PLINK
 * or Hail differ at an edge (n < 2; S = 0 or a zero expectation, which take whatever IEEE gives),
 * this text is the contract; no test compares with a PLINK binary.
 *
 * cuking_pihat_model_host: counts uint32 [num_sites][4] (hom_ref, het, hom_var, missing --
 * ignored), O(sites), on the host like cuking_site_mask_host.  INVALID_ARGUMENT: a null model,
 * with num_sites != 0 null counts, a row of more than 2^24 people.
 *
 * cuking_pihat_records_host: out[k] = z0, z1, z2, pi_hat (doubles) of records[k]'s ibs0/1/2, for
 * ANY record buffer on the host -- the buffer of cuking_compute_king as well.
 *
 * cuking_compute_pihat / _tiles: block, layout, tile ranges, counter and overflow flag exactly
 * those of cuking_compute_king: *d_result_index ends as the number of qualifying pairs whatever
 * max_results is, nothing is written past the buffer (the overflow flag is set instead),
 * max_results = 0 only counts.  Records: sample_i < sample_j, kin = (float)pi_hat, ibs0/1/2 bit
 * for bit those of a KING record of the pair; device order unspecified (the set is the contract;
 * cuking_sort_results, cuking_unrelated_set, cuking_pcrelate_pairs, cuking_ibd_pairs take the
 * buffer as it is).  The matrix-core kernels' full form with a PI_HAT epilogue (king_mfma.hip),
 * on every tile -- the filter's bound is one on KING kinship and does not apply.  Served by
 * contexts of the tiled kernel with variant 5, 6 or 7 and bitsets below 2^24 sites; every other
 * context is refused with INVALID_ARGUMENT, as are a null model, unknown flag bits and the null
 * pointers cuking_compute_king refuses.  min_pi_hat may be anything (NaN: no pair).
 * cuking_compute_pihat_host: the same records from host memory in ascending (i, j), plain
 * popcounts per pair; *num_results is the count, RESOURCE_EXHAUSTED when it exceeds max_results.
 *
 * PI_HAT assumes ONE homogeneous population: shared ancestry reads as relatedness (that is what
 * PC-Relate is for).  Out of scope: a dense PI_HAT matrix; --nudge; Hail's maf= field (pass
 * counts); per-pair missingness-specific expectations; DST, PPC and RATIO; the C++ `cuking`
 * binary; several ranks; the VALU and stream kernels. */
#define CUKING_PIHAT_UNBOUNDED 1u
typedef struct cuking_pihat_model {
  double e00, e01, e02, e11, e12;
  uint32_t sites_used;
} cuking_pihat_model;
cuking_status cuking_pihat_model_host(const uint32_t *counts, uint32_t num_sites,
                                      cuking_pihat_model *model);
cuking_status cuking_pihat_records_host(const cuking_result *records, uint64_t num_records,
                                        const cuking_pihat_model *model, uint32_t flags,
                                        double *out /* [num_records][4] */);
cuking_status cuking_compute_pihat_host(const cuking_submatrix *sm, uint32_t words_per_sample,
                                        const uint64_t *bit_sets,
                                        const cuking_pihat_model *model, float min_pi_hat,
                                        uint32_t flags, uint32_t max_results,
                                        cuking_result *results, uint32_t *num_results);
cuking_status cuking_compute_pihat(cuking_ctx *ctx, const cuking_submatrix *sm,
                                   uint32_t words_per_sample, const uint64_t *d_bit_sets,
                                   const cuking_pihat_model *model, float min_pi_hat,
                                   uint32_t flags, uint32_t max_results, cuking_result *d_results,
                                   uint32_t *d_result_index, uint32_t *d_result_overflow,
                                   void *stream);
cuking_status cuking_compute_pihat_tiles(cuking_ctx *ctx, const cuking_submatrix *sm,
                                         uint32_t words_per_sample, const uint64_t *d_bit_sets,
                                         uint64_t tile_begin, uint64_t tile_end,
                                         const cuking_pihat_model *model, float min_pi_hat,
                                         uint32_t flags, uint32_t max_results,
                                         cuking_result *d_results, uint32_t *d_result_index,
                                         uint32_t *d_result_overflow, void *stream);

/* cuking.cu:761-765 on host memory: sort by (sample_i, sample_j, kin). */
void cuking_sort_results(cuking_result *results, size_t num_results);

/* ------------------------------------------------------------------------ */
/* Test entry points: single steps of a conversion on the caller's buffers.   */
/* ------------------------------------------------------------------------ */

/* The gather of the site order ("filter_site_order") alone: for every sample s <
 * num_stored and both planes of 64 * (words_per_sample / 2) sites,
 *   d_permuted[s][plane] bit d = d_bit_set[s][plane] bit d_order[d],
 * rows words_per_sample words apart as in d_bit_set; the word behind the two planes of an
 * odd words_per_sample is not written.  d_order: a permutation of the plane's sites (the
 * padding sites of the last word among them), device memory.  gather: 0, 2 or 4 as
 * "filter_site_gather" (-1 is not taken here); CUKING_ERR_INVALID_ARGUMENT where that form
 * does not serve the width.  Every form writes the same bytes.
 * stats: 0 none; otherwise the sample statistics of a conversion of a whole diagonal block
 * of num_stored samples from that copy, into d_stats (device, stats_bytes long) -- (|Y| - |M|,
 * |H|) per plane sample, the 128 rows of the cumulative counts, the cohort's three sums and
 * the check steps, one behind the other -- 1: counted inside the byte-wide gather (gather 2 or
 * 4; what a conversion does), 2: by the separate kernel behind the gather.  The same bytes
 * either way.  layout (host, 5 words, may be null): the padded sample count, the byte offsets
 * of the rows, the sums and the steps, and the bytes needed; it is filled before stats_bytes
 * is checked.  Asynchronous on `stream`. */
cuking_status cuking_test_site_gather(cuking_ctx *ctx, const uint64_t *d_bit_set,
                                      uint32_t num_stored, uint32_t words_per_sample,
                                      const uint32_t *d_order, int gather, uint64_t *d_permuted,
                                      int stats, void *d_stats, uint64_t stats_bytes,
                                      uint64_t *layout, void *stream);

/* ------------------------------------------------------------------------ */
/* Measurement hooks (replace the StopWatch prints, cuking.cu:325-337).      */
/* ------------------------------------------------------------------------ */

/* When enabled, every launch of the pair kernel is bracketed by HIP events on
 * the stream it is launched on. */
cuking_status cuking_timing_enable(cuking_ctx *ctx, int enabled);
cuking_status cuking_timing_reset(cuking_ctx *ctx);
/* Synchronises the recorded events; returns total device milliseconds and
 * the number of launches since the last reset, for the pair kernel and for
 * the layout-preparation kernel that precedes it. */
cuking_status cuking_timing_collect(cuking_ctx *ctx, double *king_ms,
                                    uint64_t *king_launches, double *prepare_ms,
                                    uint64_t *prepare_launches);

/* Sustained shader clock while other work runs: enqueues ONE wavefront on
 * `stream` (use a stream of its own) that watches the shader-clock counter and
 * the constant 100 MHz counter for `microseconds` of wall time and then writes
 * d_ticks[0] = shader ticks, d_ticks[1] = 100 MHz ticks; clock in MHz =
 * 100 * d_ticks[0] / d_ticks[1].  It holds one wave slot of one CU meanwhile,
 * so it belongs in a pass of its own, not in a timed region. */
cuking_status cuking_clock_probe(cuking_ctx *ctx, uint64_t microseconds,
                                 uint64_t *d_ticks, void *stream);

/* ------------------------------------------------------------------------ */
/* Synthetic inputs for benchmarks (no reference counterpart).    */
/* ------------------------------------------------------------------------ */

/* Fills rows [sample_begin, sample_end) of a reference-layout bitset with
 * Hardy-Weinberg genotypes (per-site AF ~ U(0.05,0.5), 1 % missing) and the
 * planted relatives described by kind/pa/pb (device arrays of num_samples
 * u32 each; 0 founder, 1 duplicate of pa, 2 child of pa x pb).  Row 0 of
 * d_bit_set is sample_begin.  Bit-identical to oracle/synth_oracle.c.  The same
 * as cuking_synth_bitset_model with model 0. */
cuking_status cuking_synth_bitset(cuking_ctx *ctx, uint64_t seed,
                                  const uint32_t *d_kind, const uint32_t *d_pa,
                                  const uint32_t *d_pb, uint32_t sample_begin,
                                  uint32_t sample_end, uint32_t num_sites,
                                  uint32_t words_per_sample,
                                  uint64_t *d_bit_set, void *stream);

/* Named cohort models of the generator, 0 .. cuking_synth_num_models()-1 (integer
 * arithmetic only; csrc/synth.hip holds the specification, DESIGN.md 4.4 the reasons):
 *   0 "baseline"  the cohort above
 *   1 "exome"     a rare-variant spectrum: AF log-uniform on [2^-13, 1/2), 1 % missing
 *   2 "admixed"   that spectrum in two ancestries whose frequencies differ at one site
 *                 in four, and a call rate per sample: 0.5 % .. 3.5 % missing, one
 *                 sample in a hundred 10 % .. 30 %
 * cuking_synth_model_name gives "" outside the range. */
int cuking_synth_num_models(void);
const char *cuking_synth_model_name(int model);
/* cuking_synth_bitset for cohort model `model`: same arguments, same checks, and
 * CUKING_ERR_INVALID_ARGUMENT for a model outside the range.  The planted relatives
 * apply to every model.  Small per-site and per-sample tables live in scratch of the
 * context; calls on different streams are ordered by the library where one would
 * rewrite them.  Asynchronous on `stream`. */
cuking_status cuking_synth_bitset_model(cuking_ctx *ctx, int model, uint64_t seed,
                                        const uint32_t *d_kind, const uint32_t *d_pa,
                                        const uint32_t *d_pb, uint32_t sample_begin,
                                        uint32_t sample_end, uint32_t num_sites,
                                        uint32_t words_per_sample,
                                        uint64_t *d_bit_set, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CUKING_AMD_H_ */
