// Shared host/device declarations of the KING hot path (gfx950 only).
#ifndef CUKING_AMD_KING_COMMON_H_
#define CUKING_AMD_KING_COMMON_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cuking_amd.h"
#include "king_launch_plan.h"
#include "king_submatrix.h"

namespace cuking {

// ---------------------------------------------------------------------------
// Plane layout (device-internal; built by prepare_planes from the reference
// bitset of cuking.cu:507-523).
//
// For every 32-site word k and every stored sample s one uint4:
//     x = H    het and defined            (het & ~hom_var)
//     y = A    hom-alt                    (hom_var & ~het)
//     z = Hom  hom-ref or hom-alt         (~het)
//     w = D    defined (not missing)      ~(het & hom_var)
// laid out k-major: planes[k * s_stride + s].  Row samples occupy
// [0, rows_padded), column samples [col_base, col_base + cols_padded); for a
// diagonal block col_base = 0 and the samples are stored once (cuking.cu:161).
// Padding samples and padding k-words are all-zero (= everything missing),
// so they add nothing to any sum.
//
// Quad layout (kLayoutQuad, the five-product matrix-core kernel): the reference's two bit
// planes as they are, transposed: for every quad q of four consecutive 32-site
// words, plane p (0 = het, 1 = hom_var, cuking.cu:507-511) and sample s one
// uint4 holding those four words, planes[(q * 2 + p) * s_stride + s].  Half
// the bytes of the word layout (2 bits per sample and site); the kernel derives
// the A / R / H / D fragments with one three-input bit operation each.
// Padding samples and k-words have both bits set (= missing).
//
// Nibble layout (kLayoutNibble, the four-product matrix-core kernel): ONE fp4
// code per site, ready to be an MFMA operand after a single AND: for every
// group j of 32 sites and sample s one uint4 of 32 nibbles,
// planes[j * s_stride + s], site 32 j + 8 d + t in nibble t of dword d:
//     bit 0  H   het                       (E2M1 0001 = 0.5)
//     bit 1  D   defined                   (0010 = 1.0)
//     bit 2  Y   hom-ref or hom-alt        (0100 = 2.0)
//     bit 3  A   hom-alt: the SIGN of Y    (1100 = -2.0)
// i.e. hom-ref 0110, het 0011, hom-alt 1110, missing / padding 0000.  4 bits per
// sample and site = twice the bytes of the quad layout.  Behind the codes
// (at planes + k_words * s_stride) sits a het-only copy in quad form, one uint4
// per 128 sites and sample, hetq[q * s_stride + s], for the full form's hom_hom
// pass (1 bit per sample and site more).
// ---------------------------------------------------------------------------
constexpr uint32_t kLayoutWord = 0;
constexpr uint32_t kLayoutQuad = 1;
constexpr uint32_t kLayoutNibble = 2;
// ... plus what the filter kernel (king_filter.hip) reads, behind the het-only
// copy: the T2 layout -- T = hom-ref minus hom-alt alone, TWO bits per site (hom,
// hom-alt), for every unit u of 64 sites and sample s one uint4, t2[u * s_stride
// + s]: nibble t of dword d holds site 64 u + 8 d + t in bits 2-3 (code 0100 /
// 1100 = +-2.0 after `& 0xCCCCCCCC`) and site 64 u + 32 + 8 d + t in bits 0-1 as the
// OFFSET 1 + T in plain binary (hom-alt 00, het / missing / padding 01, hom-ref 10:
// the fp4 values 0 / 0.5 / 1.0 = (1 + T) / 2 after `& 0x33333333`, no shift; the
// filter kernel takes the offset out again per sample, king_filter.hip "Offset
// code"), half the bytes of the codes -- and one float2 per plane sample: (u~ =
// homozygous - missing site count + 2 S + n_A, het count), S = the sum of T over the
// sites in bits 0-1, n_A their number.
constexpr uint32_t kLayoutNibbleStats = 3;

struct PlaneGeometry {
  uint32_t num_rows, num_cols;        // block shape in samples
  uint32_t rows_padded, cols_padded;  // rounded up to the tile edge
  uint32_t col_base;                  // plane index of column sample 0
  uint32_t s_stride;                  // uint4 per k-row
  uint32_t k_words;                   // 32-site words, padded to the K chunk
  uint32_t diag;                      // rows and columns are the same samples
};

// Tiles of the block's pair space, enumerated band by band: a band is
// `band_rows` tile-rows high and is walked column-major, so that workgroups
// resident at the same time share few row/column strips (L2 reuse per XCD).
// A diagonal block only has tiles with tile_row <= tile_col.
struct TileSpace {
  uint32_t tiles_r, tiles_c;
  uint32_t band_rows;
  uint32_t diag;

  __host__ __device__ uint32_t num_bands() const {
    return (tiles_r + band_rows - 1) / band_rows;
  }
  // Tiles in band b.
  __host__ __device__ uint64_t band_tiles(uint32_t b) const {
    const uint32_t r0 = b * band_rows;
    const uint32_t h = (tiles_r - r0 < band_rows) ? tiles_r - r0 : band_rows;
    if (!diag) return (uint64_t)h * tiles_c;
    const uint32_t ncols = tiles_c - r0;  // columns r0 .. tiles_c-1
    return (uint64_t)h * (h + 1) / 2 + (uint64_t)(ncols - h) * h;
  }
  // Decodes index u inside band b.
  __host__ __device__ void decode(uint32_t b, uint64_t u, uint32_t *tr,
                                  uint32_t *tc) const {
    const uint32_t r0 = b * band_rows;
    const uint32_t h = (tiles_r - r0 < band_rows) ? tiles_r - r0 : band_rows;
    if (!diag) {
      *tc = (uint32_t)(u / h);
      *tr = r0 + (uint32_t)(u % h);
      return;
    }
    const uint64_t tri = (uint64_t)h * (h + 1) / 2;
    if (u < tri) {
      // Column r0 + c holds c + 1 tiles (rows r0 .. r0 + c).
      uint32_t c = 0;
      uint64_t before = 0;
      while (before + c + 1 <= u) {
        before += c + 1;
        ++c;
      }
      *tc = r0 + c;
      *tr = r0 + (uint32_t)(u - before);
    } else {
      const uint64_t v = u - tri;
      *tc = r0 + h + (uint32_t)(v / h);
      *tr = r0 + (uint32_t)(v % h);
    }
  }
};

// The PI_HAT form's share of the arguments (TiledArgs::pihat): the model of cuking_pihat_model,
// the threshold and the flags of the call.
struct PihatArgs {
  double e00, e01, e02, e11, e12;
  float min_pi_hat;
  uint32_t flags;
  uint32_t on;
};

// Arguments of the tiled pair kernel: what the device reads, nothing else.  The context's
// switches travel beside it (LaunchSwitches, king_launch_plan.h); the launchers turn them
// into plans and fill the launch's fields here from those.
struct TiledArgs {
  const uint4 *planes;
  PlaneGeometry geo;
  TileSpace tiles;
  const uint64_t *band_prefix;  // device; num_bands + 1 entries
  uint64_t tile_begin;          // first tile of this launch
  // Rectangle mode (rect_rows != 0): the launch covers the rect_rows tile rows
  // rect_row0 + k * rect_row_stride x the rect_cols tile columns from
  // rect_col0, enumerated in bands of band_rows rows, column-major inside a
  // band.  Used to start on the columns whose samples
  // have already arrived while the rest of the bitset is still in flight; the
  // stride lets the ranks of a node take tile rows round-robin.
  uint32_t rect_rows, rect_cols, rect_row0, rect_col0, rect_row_stride;
  uint32_t i_begin, j_begin;    // global sample index of row / column 0
  float kin_threshold;
  uint32_t max_results;
  cuking_result *results;
  uint32_t *result_index;
  uint32_t *result_overflow;
  cuking_counts *dense_counts;  // non-null: diagnostic mode, no threshold
  // Reference-layout bitset of the block (the lean kernel recounts hom/hom
  // sites from it for the pairs it emits).
  const uint64_t *bits;
  uint32_t words_per_sample;
  // Matrix-core kernel, remainder launch (king_mfma.hip): split_tiles tiles
  // from tile_begin are cut into split_wgs equal pieces of k-steps; partial
  // results are parked in split_scratch, tickets in split_counters (zero
  // between launches).  split_wgs == 0 or no scratch: never split.
  uint32_t split_tiles, split_wgs;
  // ... preceded, in the same launch, by split_whole workgroups that take one
  // whole tile each (tiles tile_begin .. tile_begin + split_whole - 1).
  uint32_t split_whole;
  uint32_t *split_scratch, *split_counters;
  // XCD-aware order (matrix-core kernel, whole-tile launches): workgroups are
  // dealt round-robin over the 8 XCDs, each with its own L2.  With xcd_chunk != 0
  // the workgroups resident on one XCD at a time hold CONSECUTIVE tiles of the
  // band order (few row/column strips per L2) instead of every eighth one:
  // xcd_chunk == 1: patches of 32 consecutive tiles, patch p on XCD p % 8
  // (workgroup b = XCD b % 8, j = b / 8 takes tile ((j / 32) * 8 + b % 8) * 32 +
  // j % 32); xcd_chunk > 1: one contiguous chunk of xcd_chunk tiles per XCD
  // (workgroup b takes tile (b % 8) * xcd_chunk + b / 8).  launch_tiles: the tiles
  // mapped by workgroup index (read only with xcd_chunk or dyn_tiles set).
  uint32_t xcd_chunk, launch_tiles;
  // Dynamic tail (matrix-core kernel, whole-tile launches of many rounds): the
  // XCDs of an MI355X run this kernel at rates 2-3 % apart and a launch's
  // workgroups are dealt to them statically, so the launch would end when the
  // slowest XCD does.  The last dyn_tiles tiles of a launch are therefore not
  // tied to a workgroup index: dyn_wgs (> dyn_tiles) workgroups behind the
  // launch_tiles statically mapped ones each take the next tile from a counter
  // (in split_counters, zero between launches) or leave at once when none is
  // left -- an XCD that gets through its static share early takes more of them.
  uint32_t dyn_tiles, dyn_wgs;
  // Quadrant mode (quad != 0): the tile space above is one of 256-sample tiles
  // (the filter variant's geometry) and the launch enumerates their four
  // 128-sample quadrants: unit t = quadrant t % 4 (row half t / 2 % 2, column
  // half t % 2) of tile t / 4.  Lets every 128-tile kernel serve a context whose
  // tile indices, tile bounds and prepared ranges are in 256-sample units.
  uint32_t quad;
  // Tile-list mode (tile_list != nullptr; matrix-core kernels): the 128-sample
  // tiles to compute are the first min(*tile_list_count, tile_list_cap) entries
  // (x = tile row, y = tile column) of a device list written by an earlier
  // kernel of the stream; workgroup b takes entries b, b + grid, ...
  const uint2 *tile_list;
  const uint32_t *tile_list_count;
  uint32_t tile_list_cap;
  // Filter variant (king_filter.hip): per-sample statistics, control words
  // (candidate count, dense-quadrant count), the candidate pairs and the
  // quadrants handed to the exact kernel instead.
  const float2 *sample_stats;
  const uint4 *t2;         // the T2 layout (king_common.h, kLayoutNibbleStats)
  uint32_t *filter_ctrl;
  unsigned long long *filter_totals;
  uint2 *cand_list;
  uint32_t cand_cap;       // entries of cand_list
  uint32_t quadrant_cap;   // candidates per quadrant beyond which it is "dense"
  uint2 *dense_list;
  uint32_t dense_cap;
  // Filter kernel, remainder of a short launch (king_filter.hip): workgroups from
  // fsplit_first on take ONE of fsplit_parts equal pieces of the k range of tile
  // fsplit_tile0 + (index - fsplit_first) / fsplit_parts of the launch; a piece
  // parks its sums in its slab, and the workgroup that delivers a tile's last
  // piece adds the others to its own (tickets: zero between launches).
  uint32_t fsplit_parts, fsplit_first, fsplit_tile0;
  float4 *fsplit_slabs;
  uint32_t *fsplit_tickets;
  // Filter kernel, check points inside the k loop (king_filter.hip, "Check points"):
  // after a number of k-steps (even) the workgroup tests its 256 x 256 sums against the
  // bound evaluated on the sites so far -- per-sample counts over that prefix, one
  // float per plane sample.  Check 1 is rigorous (every term of X is non-negative): a
  // tile none of whose pairs can still become a candidate leaves there.  Check 0
  // is a forecast (the bound scaled to the prefix) for short launches: a tile most
  // of whose quadrants look dense leaves for the exact kernel at once.  The pipeline is
  // drained at a check, so the wavefronts exchange their findings through LDS;
  // tile_done[t] = 1 tells the fallback launch that tile t of the chunk needs nothing more.
  // check_steps[k] (device memory, written by the kernel that computed the counts): k-steps
  // behind share k of kCheckShares64 from the first site on (0 = bitset too short for
  // checks); prefix_u[(x - 1) * s_stride + s]: u of plane sample s over the k-steps in front
  // of phase boundary x = 1 .. kNumCum (king_common.h phase_step).
  // Entry 0 is the forecast's (used when check0 != 0: short launches), entries 1 .. the
  // rigorous check's: every workgroup picks the same one from the threshold and the
  // cohort's mean missing and het rates (cohort_sums: samples, missing calls, het calls).
  const uint32_t *check_steps;
  const float *prefix_u;
  const unsigned long long *cohort_sums;
  // check0: 0 no forecast, 1 this is a short launch, 2 forced; check1, bits 0-7: 0 off, 1
  // automatic, 2 + k: entry k forced; bits 8-15: live
  // pairs per quadrant up to which a tile that fails the rigorous check hands them to the
  // candidate list and leaves anyway, kCheckEmitCap unless a test says otherwise; bit 16:
  // the tiles may give up at once where the cohort's sums say the bound lets every pair
  // through -- the forecast's switch, whatever the launch's length.  Both are 0 in a launch
  // without check points.
  uint32_t check0, check1;
  // Rotated tiles (king_filter.hip): 0 every tile starts at its first k-step; 1 a whole tile
  // with check points starts at the phase boundary the other tiles of its XCD are at
  // (filter_ctrl + kCtrlPos: one position word per XCD) and wraps around; 2 test hook: a
  // phase drawn from the tile's index; 3 + j test hook: phase j -- 0 as well in a launch of
  // too few tiles (king_launch_plan.h filter_plan).  rotate_min_steps: bitsets of fewer
  // k-steps are not rotated.
  uint32_t rotate, rotate_min_steps;
  uint32_t rotate_min_tiles;  // (not read by the device, always 0; kept for the layout)
  // one flag per tile of the launch chunk, directly behind the chunk's control words
  // (filter_ctrl + kCtrlChunkBytes: one memset clears both in front of a chunk)
  uint8_t *tile_done;
  // Persistent mode of the four-product kernel (king_mfma.hip), the filter's
  // fallback: when *gate != 0, workgroup b of a fixed grid takes units b, b + grid,
  // ... of the gate_count units from tile_begin on (same order as a whole-tile
  // launch: 32 consecutive units per XCD and round), skipping the quadrants of
  // tiles with skip_tiles[tile - skip_base] != 0; when *gate == 0 every workgroup
  // leaves at once.  gate == nullptr: not this mode.
  const uint32_t *gate;
  uint32_t gate_count;
  const uint8_t *skip_tiles;
  uint64_t skip_base;
  // Sample order of the kernel layout (kLayoutNibbleStats workspaces; nullptr: as
  // stored).  perm[p] = which stored sample of the block (row samples first, then the
  // columns of an off-diagonal block: the index into `bits`) sits at plane sample p, or
  // 0xFFFFFFFF for padding.  The conversion sorts the samples of a prepared range by
  // their share of missing calls (king_sort.hip), so that the few low-call-rate samples
  // of a cohort -- whose pairs the filter's bound cannot rule out -- fill a few tile rows
  // instead of spoiling every quadrant.  Pairs are enumerated in plane order (i < j there);
  // a record carries the original indices, smaller first.
  const uint32_t *perm;
  // Lazy codes (filter variant): the four-product kernel's nibble codes are converted by a
  // gated launch behind the filter kernel only if a quadrant went dense or a tile left
  // (codes_ready: device word, 1 once they are there for the prepared block).
  uint32_t *codes_ready;
  // Dense kinship matrix (cuking_compute_kin_matrix; at the END of the struct: the kernels
  // that do not read them keep their argument offsets): dense_kin non-null = no threshold,
  // no records, the float32 kinship of pair (li, lj) goes to dense_kin[li * kin_ld + lj]
  // (kin_ld in elements, 64-bit arithmetic).  kin_diag = 1 (a diagonal block, symmetric
  // output): the pairs (i, i) are stored as well -- the upper triangle WITH the diagonal;
  // the mirror kernel (launch_kin_mirror) fills the rest.  The matrix-core kernels have
  // instantiations of their own for this (king_mfma.hip, KIN), which always run on an
  // UNSORTED layout (perm is the identity and is not read); the VALU kernels store it from
  // their full form (king_device.h dense_kin_pair).
  float *dense_kin;
  uint64_t kin_ld;
  uint32_t kin_diag;
  // Kinship summary (cuking_compute_kin_summary; again at the END): the matrix-core kernels'
  // summary form (king_mfma.hip summarise_kin, instantiations of their own, unsorted layout
  // like dense_kin) adds every pair's kinship to the histogram sum_hist (sum_bins + 3 slots;
  // slot rule king_kin_summary.h with sum_lo and sum_scale = the host's (float)bins /
  // (hi - lo)) and raises the two samples' nearest-relative keys in sum_best (indexed by
  // stored sample: rows, then an off-diagonal block's columns).  Either may be null.
  unsigned long long *sum_hist, *sum_best;
  float sum_lo, sum_scale;
  uint32_t sum_bins;
  // Relative counts (cuking_compute_relative_counts; again at the END): rel_counts non-null =
  // no records; a pair whose kinship falls in band t of the rel_num ascending thresholds
  // rel_thr (band rule: king_kin_summary.h rel_band; kin_threshold = rel_thr[0]) adds 1 to
  // rel_counts[s * rel_num + t] for both its STORED samples s (rows, then an off-diagonal
  // block's columns; `perm` maps a sorted layout back).  The thresholded path with counting
  // forms of its own: king_refine_count_kernel (king_filter.hip) and the matrix-core
  // kernels' count_relatives epilogue (king_mfma.hip), chosen on the host.
  uint32_t *rel_counts;
  uint32_t rel_num;
  float rel_thr[CUKING_REL_THRESHOLDS_MAX];
  // Site order (king_sort.hip "Site order"; again at the END): non-null = the T2 layout and
  // the per-sample counts hold the sites sorted by the X they contribute to an unrelated
  // pair, and this is the cohort's measured curve (SiteCurve) the filter kernel takes the
  // share in front of its rigorous check from.  nullptr: stored order, the linear rule.
  const struct SiteCurve *site_curve;
  // (1: a launch of such a layout that "filter_rotate" 1 would rotate keeps that switch, its
  //  tiles rotate inside the head of the order -- king_filter.hip plan_checks, "head lap";
  //  0: launch_filter turns that rotation off.  "filter_site_order" 2, and -1 by
  //  kSiteOrderAutoLap below)
  uint32_t site_lap;
  // PI_HAT records (cuking_compute_pihat; again at the END): pihat.on != 0 = the matrix-core
  // kernels' full form with the PI_HAT epilogue (king_mfma.hip emit_pihat_records,
  // instantiations of their own): a pair is appended iff pihat_of_counts() of its IBS counts
  // (king_pihat.h; the model by value) > pihat.min_pi_hat, and the record's kin field holds that
  // float.  kin_threshold is not read.
  struct PihatArgs pihat;
};

// Prefix statistics: the k-steps (of 256 sites) a check may sit behind, as shares of the
// bitset in 1/64ths -- the per-sample prefix counts are computed for every entry when
// the layout is prepared, a launch picks the entries its threshold calls for.
// Live pairs per quadrant a tile may hand to the candidate list at the rigorous check
// (3.4 ns of recount each at 100k sites; the k-steps saved are ~50 us of a tile).
constexpr uint32_t kCheckEmitCap = 64;
constexpr uint32_t kNumCheckShares = 8;
constexpr uint32_t kCheckShares64[kNumCheckShares] = {8, 50, 53, 56, 58, 60, 61, 62};
// The k-steps of a bitset in kNumPhases PHASES: phase x is k-steps [phase_step(x), phase_step(x + 1)).
// A tile may start its k loop at any phase boundary and wrap around (king_filter.hip,
// "Rotated tiles": the tiles an XCD holds at a time read the same k-steps at the same time,
// whenever each of them started), so the per-sample prefix counts are kept CUMULATIVE at
// every phase boundary: u over phases [a, b) is the difference of two of them.
constexpr uint32_t kNumPhases = 128;  // (a multiple of 64: the checks' shares are 64ths)
constexpr uint32_t kPhasesPerShare = kNumPhases / 64;
constexpr uint32_t kNumCum = kNumPhases - 1;  // inner boundaries (0 is zero, the last the total)
__host__ __device__ inline uint32_t phase_step(uint32_t all_steps, uint32_t x) {
  return (uint32_t)((uint64_t)all_steps * x / kNumPhases);
}
// Site order (king_sort.hip): the cohort's curve of X over the layout's site order, left by
// the conversion beside the cohort's sums.  cum[x] = the sum over the sites in front of phase
// boundary x + 1 (cum[kNumPhases - 1]: over all sites) of the site's weight, the sum of
// (g - g')^2 over the unordered pairs of samples both defined there,
//     w = ref het + het alt + 4 ref alt        (exact integers from the site's counts);
// a random pair's expected X over a range of sites is that range's weight / pairs of samples.
// sigma: the standard deviation of the bound's kinship for such a pair from the SAME counts,
// sqrt(sum over the sites of Var (g - g')^2) / (4 mean |H|) -- on a flat spectrum near the
// 1 / sqrt(sites) of bound_level() (king_filter.hip), on an exome-like one several times that.
// het_calls, missing_calls: the cohort's totals from the same counts (what bound_level() takes
// its mean from, there from a sample of the samples).
// Automatic ("filter_site_order" -1): blocks of at least this many 256-sample tiles -- the
// gather grows with the samples, what it saves with their square; measured at 100k sites and a
// gain of 8/64 (profiles/r18_site_order.txt F): the order still loses 0.1 of 28.7 ms at 16,290
// tiles and wins 8.4 of 131 at 76,636, the floor sits between -- AND a curve that forecasts a check at least
// kSiteOrderMinGain 64ths earlier than stored order's (site_order_forecast()); a block that
// fails the second test has paid the counts, the sort and one host wait, and keeps stored
// order and its rotated tiles.
constexpr uint64_t kSiteOrderMinTiles = 24576;
constexpr uint32_t kSiteOrderMinGain = 2;
constexpr uint32_t kSiteOrderNoTrust = 15;  // conversions of a block that trust its last "no"
// Automatic mode takes the head lap (king_filter.hip plan_checks) wherever it takes the order
// and the launch would rotate a stored-order layout: profiles/r20_head_lap.txt.
constexpr bool kSiteOrderAutoLap = true;
struct SiteCurve {
  unsigned long long cum[kNumPhases];
  unsigned long long het_calls, missing_calls;
  float sigma;
  uint32_t pad[11];
};
static_assert(sizeof(SiteCurve) % 64 == 0, "whole 64-byte lines");
// The share of the k-steps (in 64ths) a tile that starts at phase boundary `phase` needs in
// front of its rigorous check when the sites are in the curve's order: candidate `share64`
// will do when the weight of the phases [phase, phase + share64 kPhasesPerShare) (around the
// end) is at least `need` of all weight -- need = (1 - 2 thr) / (1 - 2 kappa), the share of
// X an unrelated pair must have shown (king_filter.hip "Check points"; in stored order X is
// taken to grow linearly and need IS the share).
// site_curve_mass: that weight as a share of all weight (0 for a cohort without any).
__host__ __device__ inline float site_curve_mass(const unsigned long long *cum, uint32_t phase,
                                                 uint32_t share64) {
  const uint32_t hi = phase + share64 * kPhasesPerShare;  // (< 2 kNumPhases)
  auto front = [&](uint32_t x) { return x == 0 ? 0ull : cum[x - 1]; };
  const unsigned long long all = cum[kNumPhases - 1];
  const unsigned long long got = hi <= kNumPhases ? front(hi) - front(phase)
                                                  : (all - front(phase)) + front(hi - kNumPhases);
  return all != 0 ? (float)got / (float)all : 0.f;
}
__host__ __device__ inline bool site_curve_covers(const unsigned long long *cum, uint32_t phase,
                                                  uint32_t share64, float need) {
  return site_curve_mass(cum, phase, share64) >= need;
}
// k-steps (of 256 sites) behind share k for a bitset of `all_steps` k-steps, counted from
// the bitset's first site; 0 when the bitset is too short for a check to pay.
__host__ __device__ inline uint32_t check_step_of(uint32_t all_steps, uint32_t k,
                                                  uint32_t min_steps = 64) {
  if (all_steps < min_steps) return 0;
  return phase_step(all_steps, kCheckShares64[k] * kPhasesPerShare);
}
// Remainder splitting: at most this many pieces per launch (one per CU), a slab of
// 256 x 256 float sums and a ticket word each.
constexpr uint32_t kFilterSplitSlabs = 256;
constexpr size_t kFilterSlabBytes = 256 * 256 * sizeof(float);
constexpr size_t kFilterTicketBytes = kFilterSplitSlabs * sizeof(uint32_t);
// Bytes of the plane workspace for a geometry.
__host__ __device__ inline size_t plane_bytes(const PlaneGeometry &g,
                                              uint32_t layout) {
  // word layout: 16 B per 32-site word and sample; quad layout: 2 x 16 B per
  // four words and sample; nibble layout: 16 B per 32 sites and sample.
  const size_t base = (size_t)g.k_words * g.s_stride * (layout == kLayoutQuad ? 8 : 16);
  if (layout == kLayoutNibble) return base + base / 4;  // + the het-only copy
  if (layout == kLayoutNibbleStats)
    return base + base / 4 + base / 2 + (size_t)g.s_stride * sizeof(float2) +
           (size_t)g.s_stride * kNumCum * sizeof(float) + 64 + 64 +
           // control block, perm, statistics before the sort, the sort's four arrays
           64 + (size_t)g.s_stride * (4 + 8 + 4 * (kNumCum + 1) + 16) +
           // the site order's curve, behind everything else
           sizeof(SiteCurve);
  return base;
}
// Where the T2 layout and the per-sample statistics of kLayoutNibbleStats start
// (k_words is a multiple of 8: whole uint4 either way).
__host__ __device__ inline const uint4 *plane_t2(const uint4 *planes, const PlaneGeometry &g) {
  return planes + (size_t)g.k_words * g.s_stride * 5 / 4;
}
__host__ __device__ inline const float2 *plane_stats(const uint4 *planes, const PlaneGeometry &g) {
  return reinterpret_cast<const float2 *>(planes + (size_t)g.k_words * g.s_stride * 7 / 4);
}
// ... behind them the cumulative counts (kNumCum x s_stride floats) and the cohort's
// sums (three u64: samples counted, missing calls, het calls; s_stride is a multiple of
// the tile edge, so everything stays 16-byte aligned), then the k-steps behind each share
// as the prefix counts were computed for (kNumCheckShares u32).
__host__ __device__ inline const float *plane_prefix_u(const uint4 *planes, const PlaneGeometry &g) {
  return reinterpret_cast<const float *>(plane_stats(planes, g) + g.s_stride);
}
__host__ __device__ inline const unsigned long long *plane_cohort_sums(const uint4 *planes,
                                                                       const PlaneGeometry &g) {
  return reinterpret_cast<const unsigned long long *>(plane_prefix_u(planes, g) +
                                                      (size_t)g.s_stride * kNumCum);
}

// One compiled shape of the tiled kernel.
struct TiledVariant {
  const char *name;
  uint32_t tile;      // samples per tile edge
  uint32_t k_chunk;   // 32-site words staged per LDS buffer
  uint32_t threads;   // workgroup size
  uint32_t lds_bytes; // dynamic LDS
  uint32_t layout;    // kLayoutWord / kLayoutQuad
};

// The matrix-core variant accumulates in float32: exact while every sum stays
// below 2^24.
constexpr uint32_t kMfmaMaxSites = 1u << 24;

constexpr int kNumTiledVariants = 8;
constexpr int kMfmaVariant = 5;    // five plane products, quad layout
constexpr int kMfmaN4Variant = 6;  // four plane products, nibble layout (king_mfma.hip)
// The four-product variant decides kinship on the integer num = hi + hj - 2 dd
// + 2 q, which equals the reference's float expression while every partial sum
// of that is exact, i.e. below 2^22 sites (include/cuking_amd.h, numerics
// contract); wider bitsets take the five-product variant.
constexpr uint32_t kMfmaN4MaxSites = 1u << 22;
// The filter kernel's sums (king_filter.hip "Offset code") in units of their steps: the
// accumulators count quarters up to 2.5 per site, u~_i - 8 acc is an integer up to 3.5
// per site, the value tested one up to 4 per site -- each an exact float up to 2^24.  The
// per-sample u~ = u + 2 S + n_A over any set of sites is at most 2.5 per site, and so is every
// partial of the range differences the kernel forms from the cumulative table (king_filter.hip
// prefix_u_of: a wrapped range is (total - front) + wrapped end, never total + wrapped end,
// which would reach 5 per site).
static_assert(4ull * kMfmaN4MaxSites <= (1ull << 24), "filter kernel: exact float sums");
constexpr int kMfmaN4Stages = 5;
constexpr uint32_t kMfmaN4LdsBytes = kMfmaN4Stages * 2 * 2 * 4 * 128 * 16;  // 5 x 32 KiB
static_assert(kMfmaN4LdsBytes <= 160 * 1024, "LDS of one CU");
// One plane product T_i.T_j per pair as a rigorous upper bound on kinship, exact
// recount of the few pairs it lets through (king_filter.hip); 256-sample tiles.
constexpr int kMfmaFilterVariant = 7;
constexpr uint32_t kFilterTile = 256;
constexpr uint32_t kFilterLdsBytes = 5 * 2 * 2 * 2 * 256 * 16;  // 5 x 32 KiB
static_assert(kFilterLdsBytes <= 160 * 1024, "LDS of one CU");
// Per launch chunk: at most this many 256-tiles (bounds the dense-quadrant list).
constexpr uint32_t kFilterChunkTiles = 1u << 17;
// Candidate pairs per chunk: 64 per quadrant of a full chunk.  (2^20 until the missing-rate
// curve, profiles/r03_missing_curve.txt: at configs[2] with 7 % missing the bound lets 4 x 10^6
// pairs through -- 14 ms of recounts -- but the list was full after the first million and
// 230,000 quadrants went to the exact kernel instead, 512 ms for a 160 ms pass.)
constexpr uint32_t kFilterCandCap = 1u << 25;
// Candidates per 128 x 128 quadrant beyond which the quadrant goes to the exact
// kernel: one wavefront per candidate costs 3.4 ns of chip time at 100k sites
// (1.65 M candidates in 5.6 ms), the four-product kernel 1.85 us per quadrant --
// break-even near 540, whatever the site count (both are linear in it;
// profiles/r03_filter_curve.txt).
constexpr uint32_t kFilterQuadrantCap = 384;
constexpr size_t kFilterCtrlBytes = 256;
// Control words (uint32 indices into filter_ctrl).  Zeroed in front of every launch
// chunk (kCtrlChunkBytes): 0 candidates of the chunk, 1 dense quadrants of the chunk
// (list slots), 2 dynamic-tail counter, 3 quadrants finished, 4 quadrants of tiles that
// left for the exact kernel at check 0, 5 "every remaining tile leaves" (most quadrants
// so far went dense), 6 gate of the fallback launch (some tile left).  Running totals
// since the scratch was allocated (u64 each, behind the tile flags: TiledArgs::
// filter_totals): 0 candidates, 1 quadrants handed to the exact kernel, 2 tiles that left
// at the rigorous check, 3 tiles that started at another phase than the first.
constexpr uint32_t kCtrlCand = 0, kCtrlDense = 1, kCtrlDyn = 2, kCtrlFinished = 3,
                   kCtrlLeft = 4, kCtrlAllLeave = 5, kCtrlGate = 6;
// ... and where the tiles of each XCD are (rotated tiles, king_filter.hip): word 8 + x: the
// 100 MHz counter's ticks per k-step x 16 as a tile of XCD x last measured them; from byte
// 64 on, per XCD kPosSlots u64 = (k-step, counted on through the tiles, a tile of the XCD
// had reached) << 32 | (when: low word of that counter) -- a tile writes slot (its
// workgroup's turn on the XCD) mod kPosSlots at its segment ends, a new tile joins the most
// advanced of them.
constexpr uint32_t kCtrlStepTicks = 8, kCtrlPos = 16, kPosSlots = 16;
constexpr size_t kCtrlChunkBytes = (kCtrlPos + 8 * kPosSlots * 2) * 4;
constexpr uint32_t kTotalCand = 0, kTotalDense = 1, kTotalEarly = 2, kTotalRotated = 3;
constexpr uint32_t kNumTotals = 4;
__host__ __device__ inline const uint32_t *plane_check_steps(const uint4 *planes,
                                                             const PlaneGeometry &g) {
  return reinterpret_cast<const uint32_t *>(plane_cohort_sums(planes, g) + 8);
}
// ... one control block (16 u32; word 0: codes_ready), then the sample order and what
// building it needs, every array s_stride entries long: perm (u32), the statistics in
// stored order before the sort (float2 (u, |H|), then kNumCum + 1 floats: u~ cumulative
// and over all sites), keys in / out and values in / out of the sort (u32 each).
__host__ __device__ inline uint32_t *plane_flags(const uint4 *planes, const PlaneGeometry &g) {
  return const_cast<uint32_t *>(plane_check_steps(planes, g)) + 16;
}
__host__ __device__ inline uint32_t *plane_perm(const uint4 *planes, const PlaneGeometry &g) {
  return plane_flags(planes, g) + 16;
}
__host__ __device__ inline float2 *plane_tmp_stats(const uint4 *planes, const PlaneGeometry &g) {
  return reinterpret_cast<float2 *>(plane_perm(planes, g) + g.s_stride);
}
__host__ __device__ inline float *plane_tmp_prefix(const uint4 *planes, const PlaneGeometry &g) {
  return reinterpret_cast<float *>(plane_tmp_stats(planes, g) + g.s_stride);
}
__host__ __device__ inline uint32_t *plane_sort_words(const uint4 *planes, const PlaneGeometry &g) {
  return reinterpret_cast<uint32_t *>(plane_tmp_prefix(planes, g) +
                                      (size_t)g.s_stride * (kNumCum + 1));
}
// ... and behind the sort's arrays the site order's curve.
__host__ __device__ inline SiteCurve *plane_site_curve(const uint4 *planes, const PlaneGeometry &g) {
  return reinterpret_cast<SiteCurve *>(plane_sort_words(planes, g) + 4 * (size_t)g.s_stride);
}
constexpr uint32_t kNoSample = 0xFFFFFFFFu;

// Scratch of one stream: the chunk's control words and one flag per tile of a launch chunk
// (cleared together in front of every chunk), the running totals, tickets, the candidate
// list, the dense-quadrant list, the remainder slabs.  The lists are sized for the block the
// scratch serves (`tiles` 256-sample tiles in its enumeration): 64 candidates per quadrant
// of a chunk, at most kFilterCandCap.
struct FilterScratchLayout {
  size_t tile_done, totals, tickets, cand, dense, slabs, bytes;
  uint32_t chunk_tiles, cand_entries;
};
inline FilterScratchLayout filter_scratch_layout(uint64_t tiles) {
  FilterScratchLayout l;
  l.chunk_tiles = (uint32_t)(tiles < kFilterChunkTiles ? (tiles ? tiles : 1) : kFilterChunkTiles);
  const uint64_t cand = (uint64_t)l.chunk_tiles * 4 * 64;
  l.cand_entries = (uint32_t)(cand < kFilterCandCap ? cand : kFilterCandCap);
  auto up = [](size_t x) { return (x + 255) / 256 * 256; };
  l.tile_done = kCtrlChunkBytes;
  l.totals = up(l.tile_done + l.chunk_tiles);
  l.tickets = l.totals + kFilterCtrlBytes;
  l.cand = l.tickets + kFilterTicketBytes;
  l.dense = l.cand + up((size_t)l.cand_entries * sizeof(uint2));
  l.slabs = l.dense + up((size_t)l.chunk_tiles * 4 * sizeof(uint2));
  l.bytes = l.slabs + kFilterSplitSlabs * kFilterSlabBytes;
  return l;
}
inline bool is_mfma_variant(int v) {
  return v == kMfmaVariant || v == kMfmaN4Variant || v == kMfmaFilterVariant;
}
// LDS stages of the five-product kernel's full form (16 KiB each, king_mfma.hip; the
// lean form has kStagesPaired): stage s + kMfmaStages - 1 is requested while stage s is
// multiplied, i.e. kMfmaStages - 2 k-steps (~1.4 us each) of HBM latency are covered.
constexpr int kMfmaStages = 6;
constexpr uint32_t kMfmaLdsBytes = kMfmaStages * 2 * 2 * 2 * 128 * 16;
// The full form parks its fifth sum (64 registers per lane) behind the stages.
constexpr uint32_t kMfmaParkBytes = 4 * 64 * 64 * 4;
static_assert(kMfmaLdsBytes + kMfmaParkBytes <= 160 * 1024, "LDS of one CU");
const TiledVariant &tiled_variant(int v);
// Enqueues tiles [args.tile_begin, args.tile_begin + num_tiles) of a geometry whose tile
// edge is `plan_tile`, for the call form sw.form (king_launch_plan.h kCallForms: the form
// says which kernels can serve it and which k loops; no launcher looks at the output
// pointers to find out).  `variant`: the kernel variant that runs.  Where its tile edge is
// half the geometry's -- the filter variant's 256-sample tiles under a 128-tile kernel: a
// wide bitset, or a call the filter does not run for (sw.filter_runs, king_abi.hip
// filter_runs: the same answer decides whether the four-product kernel's codes are converted
// up front) -- the tiles go out as their quadrants; this is the one place that says so.
// full = accumulate all five sums for every pair (needed for the diagnostic
// counts; chosen when nearly every pair is expected to pass the threshold);
// otherwise the lean form: four sums in the main loop, IBS2 recounted for
// emitted pairs only.  Same records either way.
// `args`: the call's base arguments (no launch mode set: whole tiles in plain order);
// every launcher fills the fields of its own modes from its plan.
hipError_t launch_tiled(int variant, uint32_t plan_tile, bool full, const TiledArgs &args,
                        const LaunchSwitches &sw, uint64_t num_tiles, hipStream_t stream);
// The matrix-core kernels (king_mfma.hip), every form of them, reached through launch_tiled:
// the k loop of the four-product (nibble) or the five-product kernel and the epilogue of
// sw.form -- records, counts, a stored or a reduced float32 kinship of every pair, relative
// counts, PI_HAT records -- under one launch plan (chunking, XCD order, dynamic tail,
// remainder split).  Refuses a form with the k loop it does not have (kernel_form) and
// device arguments that lack what the form's epilogue reads.  lds_bytes: the variant
// table's figure, which only the five-product full form goes by.
hipError_t launch_mfma(bool full, bool nibble, const TiledArgs &args, const LaunchSwitches &sw,
                       uint64_t num_tiles, uint32_t lds_bytes, hipStream_t stream);
// Symmetric fill of an n x n kinship matrix whose upper triangle (and diagonal) is there:
// kin[j * ld + i] = kin[i * ld + j] for i < j, tile-wise through LDS, reads and writes
// coalesced.  Runs behind the pair kernel on the same stream.
hipError_t launch_kin_mirror(float *d_kin, uint64_t ld, uint32_t n, hipStream_t stream);
// The four-product kernel, lean form, over the first min(*count, cap) entries of the device
// list `list` (TiledArgs::tile_list) with `grid` workgroups.  This and the next one run
// behind the filter kernel, for the forms it serves: `form` is records or relative counts.
hipError_t launch_mfma_list(CallForm form, const TiledArgs &args, const uint2 *list,
                            const uint32_t *count, uint32_t cap, uint32_t grid,
                            hipStream_t stream);
// The four-product kernel, lean form, persistent mode (TiledArgs::gate): `grid`
// workgroups walk num_units units from args.tile_begin on, if *gate != 0, skipping the
// quadrants of tiles with skip_tiles[tile - skip_base] != 0.
hipError_t launch_mfma_gated(CallForm form, const TiledArgs &args, uint64_t num_units,
                             const uint32_t *gate, const uint8_t *skip_tiles, uint64_t skip_base,
                             uint32_t grid, hipStream_t stream);
// The filter variant (king_filter.hip): num_tiles 256-sample tiles from
// args.tile_begin; needs args.filter_ctrl etc. (king_abi.hip: filter scratch).  sw.form says
// whether its exact kernels append records or count relatives.
hipError_t launch_filter(const TiledArgs &args, const LaunchSwitches &sw, uint64_t num_tiles,
                         hipStream_t stream);
// Quadrant mode (TiledArgs::quad): the launch of *num_units 256-sample tiles from
// a->tile_begin as their 128-sample quadrants.
inline void to_quadrants(TiledArgs *a, uint64_t *num_units) {
  a->quad = 1;
  a->tile_begin *= 4;
  *num_units *= 4;
}
// Statistics of plane samples [s_begin, s_end) of a kLayoutNibbleStats workspace.
hipError_t launch_sample_stats(const uint64_t *d_bit_sets, uint32_t words_per_sample,
                               const PlaneGeometry &geo, uint4 *d_planes, uint32_t s_begin,
                               uint32_t s_end, hipStream_t stream);
// Where the statistics go: (|Y| - |M|, |H|) per plane sample, the kNumCum + 1 rows of the
// cumulative u~ (s_stride apart), the cohort's three sums and the check steps -- of a
// workspace (stats_arrays) or a caller's (tests).
struct SampleStatsArrays {
  float2 *stats;
  float *cum;
  unsigned long long *sums;
  uint32_t *steps;
};
inline SampleStatsArrays stats_arrays(const PlaneGeometry &geo, uint4 *d_planes) {
  return {plane_tmp_stats(d_planes, geo), plane_tmp_prefix(d_planes, geo),
          const_cast<unsigned long long *>(plane_cohort_sums(d_planes, geo)),
          const_cast<uint32_t *>(plane_check_steps(d_planes, geo))};
}
hipError_t launch_sample_stats_to(const uint64_t *d_bit_sets, uint32_t words_per_sample,
                                  const PlaneGeometry &geo, const SampleStatsArrays &to,
                                  uint32_t s_begin, uint32_t s_end, hipStream_t stream);
// Test hook, process-wide: bitsets of fewer k-steps get no check points (default 64).
void set_filter_check_min_steps(uint32_t steps);
uint32_t filter_check_min_steps();
// The sample order of plane samples [s_begin, s_end) of a kLayoutNibbleStats workspace
// (king_sort.hip): statistics in stored order -> keys -> stable sort (or none) -> perm and
// the statistics in plane order.  `sort_temp` / `sort_temp_bytes`: device scratch of at
// least sort_temp_bytes_for(s_end - s_begin).
size_t sort_temp_bytes_for(uint32_t n);
hipError_t launch_sample_order(const PlaneGeometry &geo, uint32_t words_per_sample,
                               uint4 *d_planes, uint32_t s_begin, uint32_t s_end, bool sort,
                               void *sort_temp, size_t sort_temp_bytes, hipStream_t stream);
// Site order (king_sort.hip): the scratch a conversion with the order on needs for a block of
// `num_stored` stored samples (0: the order cannot be built for this width -- a sample's two
// planes must fit the gather's LDS), and the conversion's first steps: site counts, weights,
// stable sort, the bitset with every sample's sites in that order at the scratch's
// `permuted` (same shape as d_bit_sets: what sample_stats_kernel and the T2 conversion then
// read instead), and the curve at `curve`.
// launch_site_order: counts, weights, sort and curve; launch_site_permute: the gather -- two
// calls, so that the host may read the curve in between and keep stored order after all.
struct SiteOrderScratch {
  size_t counts, keys, vals, sort_temp, sort_temp_bytes, permuted, bytes;
};
SiteOrderScratch site_order_scratch(uint32_t num_stored, uint32_t words_per_sample);
hipError_t launch_site_order(const uint64_t *d_bit_sets, uint32_t num_stored,
                             uint32_t words_per_sample, const PlaneGeometry &geo, void *d_scratch,
                             const SiteOrderScratch &layout, SiteCurve *d_curve,
                             hipStream_t stream);
// `gather`: what site_gather_pick() made of "filter_site_gather" for this width -- 4 or 2
// samples per LDS field (gather_sites_kernel, king_site_gather.h), 0 the ballot kernel
// (permute_sites_kernel); -1 from site_gather_pick: the option forces a form that does not
// fit.  The kernels write the same bytes.
// `fused` (gather 4 or 2 only, a whole diagonal block: plane sample = stored sample): the
// gather also leaves what sample_stats_kernel would leave for plane samples [0, num_stored)
// of a conversion of plane samples [0, s_end) -- the same bytes, the cohort's sums from the
// same samples --, counted on the output words while a wavefront holds them; the padding
// samples behind them stay with launch_sample_stats.
int site_gather_pick(int option, uint32_t words_per_sample);
struct SiteGatherStats {
  SampleStatsArrays to;
  PlaneGeometry geo;
  uint32_t s_end;
};
hipError_t launch_site_permute(const uint64_t *d_bit_sets, uint32_t num_stored,
                               uint32_t words_per_sample, void *d_scratch,
                               const SiteOrderScratch &layout, int gather,
                               const SiteGatherStats *fused, hipStream_t stream);
// The gather alone: d_permuted[sample][plane][d] = d_bit_sets[sample][plane][d_order[d]] for
// the 64 * (words_per_sample / 2) sites of a plane (d_order: a permutation of them).
hipError_t launch_site_gather(const uint64_t *d_bit_sets, uint32_t num_stored,
                              uint32_t words_per_sample, const uint32_t *d_order,
                              uint64_t *d_permuted, int gather, const SiteGatherStats *fused,
                              hipStream_t stream);
// What a curve forecasts for the rigorous check of an unrotated tile at threshold `thr`, in
// 64ths of the k-steps (0: no check up to 62/64): `stored64` by the linear rule of stored
// order, `order64` from the curve -- the arithmetic of the filter kernel (king_filter.hip
// plan_checks, launch_verdict), with the cohort's rates from all samples instead of a sample
// of them.  `verdict_first`: the launch-wide verdict lets every tile leave before it starts.
struct SiteOrderForecast {
  uint32_t stored64, order64;
  bool verdict_first;
};
SiteOrderForecast site_order_forecast(const SiteCurve &curve, uint32_t num_stored,
                                      uint32_t k_words, float thr);
// Codes (+ het-only copy) and / or T2 of plane tiles [s_tile_begin, s_tile_end) of a
// nibble workspace; `gate` != nullptr: only if a quadrant went dense or a tile left
// (filter control words) and the codes are not there yet (*ready == 0).
hipError_t launch_prepare_nibbles(bool codes, bool t2, const uint64_t *d_bit_sets,
                                  uint32_t words_per_sample, const PlaneGeometry &geo,
                                  uint4 *d_planes, const uint32_t *perm, uint32_t s_tile_begin,
                                  uint32_t s_tile_end, const uint32_t *gate,
                                  const uint32_t *ready, hipStream_t stream);
// *ready = 1 if the gate is open (behind a gated launch_prepare_nibbles).
hipError_t launch_mark_codes_ready(const uint32_t *gate, uint32_t *ready, hipStream_t stream);
// Bytes of split scratch (counters, then slabs) for `wgs` workgroups, and of
// the counter part alone (the only part that must start out zero).
size_t mfma_split_scratch_bytes(uint32_t wgs);
size_t mfma_split_counter_bytes(uint32_t wgs);

// Test hook: cap the workgroups per launch (0 = hardware limit only), and the cap set.
void set_max_blocks_per_launch(uint64_t blocks);
uint64_t max_blocks_override();

// Converts plane-sample tiles [s_tile_begin, s_tile_end) (units of 64 plane
// samples) of the block.
hipError_t launch_prepare_planes(uint32_t layout, const uint64_t *d_bit_sets,
                                 uint32_t words_per_sample,
                                 const PlaneGeometry &geo, uint4 *d_planes,
                                 uint32_t s_tile_begin, uint32_t s_tile_end,
                                 hipStream_t stream);

hipError_t launch_stream(const cuking_submatrix &sm, uint32_t words_per_sample,
                         const uint64_t *d_bit_sets, float kin_threshold,
                         uint32_t max_results, cuking_result *d_results,
                         uint32_t *d_result_index, uint32_t *d_result_overflow,
                         cuking_counts *d_dense_counts, float *d_dense_kin, uint64_t kin_ld,
                         uint32_t kin_diag, hipStream_t stream);

hipError_t launch_pack(const cuking_submatrix &sm, uint32_t words_per_sample,
                       uint64_t *d_bit_set, const int64_t *d_row_idx,
                       const int64_t *d_col_idx, const int32_t *d_n_alt,
                       size_t num_triples, uint32_t *d_status,
                       hipStream_t stream);

hipError_t launch_pack_compact(uint32_t words_per_sample, uint32_t num_samples,
                               uint64_t *d_bit_set, const uint32_t *d_site,
                               const uint32_t *d_sample_alt, size_t num_triples,
                               uint32_t *d_status, hipStream_t stream);

// PLINK .bed rows -> bitset (king_bed.hip): sites [site_begin, site_end) of the block's stored
// samples, d_bed_rows = the row of site_begin; arguments already checked (king_host.h
// cuking_check_bed_args).  Plain stores, no status word: every code is legal.
hipError_t launch_pack_bed(const cuking_submatrix &sm, uint32_t words_per_sample,
                           uint64_t *d_bit_set, const uint8_t *d_bed_rows, uint64_t row_bytes,
                           uint32_t site_begin, uint32_t site_end, hipStream_t stream);

// Site QC (king_site_qc.hip; arguments already checked, king_host.h).  launch_site_counts ADDS
// into d_counts [64 P][4], launch_sample_counts overwrites d_counts [num_stored][4];
// launch_compact_sites reads d_table, the device copy of build_compact_table's output
// (king_site_qc.h).  site_counts_block_samples: the most samples one workgroup of the count
// kernel adds up between two flushes of its bit-sliced counters.
hipError_t launch_site_counts(const uint64_t *d_bit_set, uint32_t num_stored,
                              uint32_t words_per_sample, uint32_t *d_counts, hipStream_t stream);
hipError_t launch_sample_counts(const uint64_t *d_bit_set, uint32_t num_stored,
                                uint32_t words_per_sample, uint32_t num_sites,
                                uint32_t *d_counts, hipStream_t stream);
hipError_t launch_compact_sites(const uint64_t *d_in, uint32_t num_stored,
                                uint32_t words_per_sample_in, const void *d_table,
                                uint32_t num_kept, uint64_t *d_out,
                                uint32_t words_per_sample_out, hipStream_t stream);
uint32_t site_counts_block_samples();

// LD pruning (king_ld.hip; arguments already checked, king_host.h).  launch_transpose_sites
// writes every word of d_site_bits [num_sites][2][Q] once; launch_ld_edges ADDS the number of
// edges to *d_count (zeroed by the caller, on the stream) and stores the records whose slot is
// below max_records.
hipError_t launch_transpose_sites(const uint64_t *d_bit_set, uint32_t num_stored,
                                  uint32_t words_per_sample, uint32_t num_sites,
                                  uint64_t *d_site_bits, hipStream_t stream);
hipError_t launch_ld_edges(const uint64_t *d_site_bits, uint32_t num_sites, uint32_t num_stored,
                           uint32_t window, float r2_threshold, const int32_t *d_group,
                           cuking_result *d_records, uint64_t max_records,
                           unsigned long long *d_count, hipStream_t stream);

// Genotype matrix products (king_geno.hip; arguments already checked, king_host.h).  Plain
// stores into d_out[r][0 .. num_rhs) of every row; num_cols == 0 stores zeros.
hipError_t launch_geno_matmul(const uint64_t *d_bits, uint32_t num_rows, uint32_t words_per_row,
                              uint32_t num_cols, const float *d_table, bool per_row,
                              const float *d_b, uint32_t ldb, uint32_t num_rhs, float *d_out,
                              uint32_t ldo, hipStream_t stream);

// PC-Relate (king_pcrelate.hip; arguments already checked, king_host.h).  Plain stores into
// d_out[i - i_begin][j - j_begin] of every pair of `block`; num_sites == 0 stores NaN.
hipError_t launch_pcrelate_matrix(const uint64_t *d_bits, uint32_t words_per_sample,
                                  uint32_t num_sites, const float *d_x, uint32_t ldx,
                                  const float *d_beta, uint32_t ldbeta, uint32_t d, float lo,
                                  float hi, const cuking_submatrix &block, float *d_out,
                                  uint64_t ldo, hipStream_t stream);

// PC-Relate records (king_pcrelate_records.hip; arguments already checked, king_host.h).  ADDS
// the number of pairs of `block` with kin > min_kin to *d_count (zeroed by the caller, on the
// stream) and stores the records whose slot is below max_records; num_sites == 0 adds nothing.
hipError_t launch_pcrelate_records(const uint64_t *d_bits, uint32_t words_per_sample,
                                   uint32_t num_sites, const float *d_x, uint32_t ldx,
                                   const float *d_beta, uint32_t ldbeta, uint32_t d, float lo,
                                   float hi, const cuking_submatrix &block, float min_kin,
                                   cuking_result *d_records, uint64_t max_records,
                                   unsigned long long *d_count, hipStream_t stream);

// PC-Relate for listed pairs (king_pcrelate_pairs.hip; arguments already checked, king_host.h).
// Plain stores into d_out[0 .. num_pairs); num_sites == 0 stores the NaN rows.
hipError_t launch_pcrelate_pairs(const uint64_t *d_bits, uint32_t num_stored,
                                 uint32_t words_per_sample, uint32_t num_sites, const float *d_x,
                                 uint32_t ldx, const float *d_beta, uint32_t ldbeta, uint32_t d,
                                 float lo, float hi, const float *d_f, const void *d_pairs,
                                 uint64_t num_pairs, uint32_t pair_stride,
                                 cuking_pcrelate_pair *d_out, hipStream_t stream);

// IBD segments for listed pairs (king_ibd.hip; arguments already checked, king_host.h).
// launch_ibd_group_bits fills d_group_bits[0 .. ibd_scan_words(num_sites)) (king_ibd.h: bit s set
// iff site s starts a group; d_group may be null).  launch_ibd_pairs stores d_out[0 ..
// num_pairs) with plain stores and, when d_count is not null, ADDS the number of segments to
// *d_count (zeroed by the caller, on the stream) and stores those whose slot is below
// max_segments; num_sites == 0 stores zero rows.  bridge_sites == 0 launches the strict kernel,
// anything else the bridging instantiation; d_bridged ([num_pairs][2]) may be null.
hipError_t launch_ibd_group_bits(const int32_t *d_group, uint32_t num_sites,
                                 uint64_t *d_group_bits, hipStream_t stream);
hipError_t launch_ibd_pairs(const uint64_t *d_bits, uint32_t num_stored,
                            uint32_t words_per_sample, uint32_t num_sites,
                            const uint64_t *d_group_bits, const uint32_t *d_pos,
                            uint32_t min_sites, uint32_t min_length, uint32_t bridge_sites,
                            const void *d_pairs, uint64_t num_pairs, uint32_t pair_stride,
                            cuking_ibd_pair *d_out, uint32_t *d_bridged,
                            cuking_ibd_segment *d_segments, uint64_t max_segments,
                            unsigned long long *d_count, hipStream_t stream);
// IBD scan of a block (king_ibd_scan.hip; arguments already checked, king_host.h): ADDS the
// number of pairs of `block` with a kind-1 segment and length1 >= min_total to *d_count (zeroed
// by the caller, on the stream) and stores the records whose slot is below max_records;
// d_group_bits as above; num_sites == 0 adds nothing.
hipError_t launch_ibd_scan(const uint64_t *d_bits, uint32_t words_per_sample, uint32_t num_sites,
                           const uint64_t *d_group_bits, const uint32_t *d_pos,
                           uint32_t min_sites, uint32_t min_length,
                           const cuking_submatrix &block, uint64_t min_total,
                           cuking_ibd_pair *d_records, uint64_t max_records,
                           unsigned long long *d_count, hipStream_t stream);
// Runs of homozygosity (king_ibd.hip; arguments already checked): one row per entry of d_samples
// (null: samples 0 .. num_samples - 1), the group bits, the count and the segment list as above.
hipError_t launch_roh_samples(const uint64_t *d_bits, uint32_t num_stored,
                              uint32_t words_per_sample, uint32_t num_sites,
                              const uint64_t *d_group_bits, const uint32_t *d_pos,
                              uint32_t min_sites, uint32_t min_length, uint32_t bridge_sites,
                              const uint32_t *d_samples, uint64_t num_samples,
                              cuking_roh_sample *d_out, cuking_ibd_segment *d_segments,
                              uint64_t max_segments, unsigned long long *d_count,
                              hipStream_t stream);
// Mendelian errors (king_mendel.hip; arguments already checked): one 48-byte row per listed trio
// and, with d_error_bits, the error mask [num_trios][words_per_sample / 2]; and the column sums of
// such a mask, ADDED to d_counts [64 plane_words].
hipError_t launch_mendel_trios(const uint64_t *d_bits, uint32_t num_stored,
                               uint32_t words_per_sample, uint32_t num_sites,
                               const uint32_t *d_trios, uint64_t num_trios,
                               cuking_mendel_trio *d_out, uint64_t *d_error_bits,
                               hipStream_t stream);
hipError_t launch_mendel_site_counts(const uint64_t *d_error_bits, uint64_t num_trios,
                                     uint32_t plane_words, uint32_t *d_counts,
                                     hipStream_t stream);

// Hardy-Weinberg exact test (king_hwe.hip; arguments already checked, king_host.h): plain stores
// into d_p[0 .. num_sites) from rows [0, num_sites) of a site_counts array (16-byte aligned).
hipError_t launch_hwe_sites(const uint32_t *d_counts, uint32_t num_sites, bool midp, double *d_p,
                            hipStream_t stream);

// Cohort models of the synthetic generator (synth.hip holds the specification).  d_tables:
// synth_table_bytes() of scratch the launch fills and reads (per-site and per-sample
// tables); it must stay untouched until the launch has run.
enum { kSynthBaseline = 0, kSynthExome = 1, kSynthAdmixed = 2, kNumSynthModels = 3 };
const char *synth_model_name(int model);
size_t synth_table_bytes(uint32_t num_rows, uint32_t words_per_sample);
hipError_t launch_synth(int model, uint64_t seed, const uint32_t *d_kind,
                        const uint32_t *d_pa, const uint32_t *d_pb,
                        uint32_t sample_begin, uint32_t sample_end,
                        uint32_t num_sites, uint32_t words_per_sample,
                        void *d_tables, uint64_t *d_bit_set, hipStream_t stream);

hipError_t launch_clock_probe(uint64_t microseconds, uint64_t *d_out,
                              hipStream_t stream);

}  // namespace cuking

#endif  // CUKING_AMD_KING_COMMON_H_
