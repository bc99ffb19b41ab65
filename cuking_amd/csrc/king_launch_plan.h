// Launch planning of the pair kernels: the integer arithmetic that turns a tile count, the
// block limit and the context's switches into launches -- how many tiles go out whole, in
// which order over the XCDs, how many through the dynamic tail, which remainder is cut into
// pieces, and the grid of each launch.  Pure functions of plain integers (no HIP header, so
// that a host compiler and tests/test_launch_plan.py can read them); the launchers
// (king_mfma.hip, king_filter.hip) make a plan, copy it into the device arguments
// (TiledArgs, king_common.h) and launch.
#ifndef CUKING_AMD_KING_LAUNCH_PLAN_H_
#define CUKING_AMD_KING_LAUNCH_PLAN_H_

#include <stdint.h>

namespace cuking {

// The pair calls, by what they produce.  The entry point (king_abi.hip) names its form once;
// every layer below reads the rules of that form from kCallForms and works nothing out from
// the output pointers.  Host side only: the kernels read the pointers of TiledArgs.
enum CallForm : int {
  kFormRecords,     // records of the pairs above a kinship threshold
  kFormCounts,      // the five sums of every pair (cuking_compute_counts)
  kFormKinMatrix,   // float32 kinship of every pair, stored
  kFormKinSummary,  // float32 kinship of every pair, reduced: histogram, nearest relative
  kFormRelCounts,   // the thresholded call counted per sample, no records
  kFormPiHat,       // records of the pairs above a PI_HAT threshold
  kNumCallForms
};
// The k loop a form runs: the full one (five sums of every pair), the lean one (four sums,
// the fifth recounted where it is needed), or whichever the threshold makes cheaper.
enum KLoop : int { kLoopEither, kLoopFull, kLoopLean };
// KIN of king_mfma_kernel (king_mfma.hip): the epilogue behind the k loop.
constexpr int kRecords = 0, kKinMatrix = 1, kKinSummary = 2, kRelCounts = 3, kPiHat = 4;

struct CallFormRules {
  const char *name;  // as the messages say it
  KLoop k_loop;
  // The layout keeps the samples in stored order (no sort, TiledArgs::perm null): the form
  // writes per pair by position, or gains nothing from the filter's order.
  bool unsorted;
  // The filter's bound (one on KING kinship against a threshold) may apply; whether it does
  // depends on the variant and the threshold as well (king_abi.hip filter_runs).
  bool filter_may_run;
  // The VALU variants and the stream kernel can serve it (they store a matrix from their
  // full form); otherwise the matrix-core kernels only.
  bool valu_serves;
  int kin;  // the matrix-core kernel's KIN
};
constexpr CallFormRules kCallForms[kNumCallForms] = {
    {"records", kLoopEither, false, true, true, kRecords},
    {"counts", kLoopFull, false, false, true, kRecords},
    {"kinship matrix", kLoopLean, true, false, true, kKinMatrix},
    {"kinship summary", kLoopLean, true, false, false, kKinSummary},
    {"relative counts", kLoopLean, false, true, false, kRelCounts},
    {"pi_hat", kLoopFull, false, false, false, kPiHat},
};
static_assert(kCallForms[kNumCallForms - 1].name != nullptr, "a row for every form");
// The instantiations of king_mfma_kernel by <KIN, FULL>: the records kind has both k loops,
// every other kind one.  -1: the form does not run with that k loop.
constexpr int kNumKernelForms = 6;
constexpr int kernel_form(CallForm form, bool full) {
  if (form < 0 || form >= kNumCallForms) return -1;
  const CallFormRules &r = kCallForms[form];
  if (r.k_loop != kLoopEither && full != (r.k_loop == kLoopFull)) return -1;
  return r.kin == kRecords ? (full ? 1 : 0) : r.kin + 1;
}

// The context's switches for one call (king_abi.hip launch_switches): host side only, the
// kernels never see them.
struct LaunchSwitches {
  // Matrix-core kernels, whole-tile launches: XCD-aware order 0 off / 1 one contiguous
  // chunk per XCD / 2 patches of 32 (TiledArgs::xcd_chunk); launches of at least
  // dyn_tail_tiles tiles get a dynamic tail (0 = never; TiledArgs::dyn_tiles).
  uint32_t xcd_swizzle, dyn_tail_tiles;
  // Filter kernel.  check0 (the forecast): 0 off, 1 short launches only, 2 always;
  // check1 (the rigorous check): 0 off, 1 automatic, 2 + k entry k forced; check_emit: live
  // pairs per quadrant a tile may hand over at the rigorous check; rotate: 0 off, 1 on,
  // 2 / 3 + j test hooks, for launches of at least rotate_min_tiles tiles;
  // split_min_steps: k-steps per remainder piece, at least (0 = 8).
  uint32_t check0, check1, check_emit, rotate, rotate_min_tiles, split_min_steps;
  // The filter's bound applies to this call (filter variant, lean form, threshold inside
  // (0, 1/2)): the filter kernel runs, and the four-product kernel's codes may stay
  // unconverted until it asks for them.
  bool filter_runs;
  // The call's form: which kernels a launcher picks.
  CallForm form;
};

// One whole-tile launch: workgroup b < launch_tiles (plus padding) takes a tile by its
// index, in the order xcd_chunk says; dyn_wgs workgroups behind them take the last
// dyn_tiles tiles from a counter.  launch_tiles is only read by a kernel when xcd_chunk or
// dyn_tiles is non-zero.
struct WholeShape {
  uint64_t tiles;  // tiles the launch covers
  uint32_t launch_tiles, xcd_chunk, dyn_tiles, dyn_wgs;
  uint64_t grid;
};

// The next whole-tile launch for `want` tiles when one launch holds at most `cap`
// workgroups (it may cover fewer tiles than both).
//   xcd_swizzle: LaunchSwitches::xcd_swizzle as far as the kernel supports it.
//   dyn_min, dyn_floor: launches of at least dyn_min (0 = never) and dyn_floor tiles get a
//   dynamic tail (patch order only).
inline WholeShape whole_shape(uint64_t want, uint64_t cap, uint32_t xcd_swizzle, uint64_t dyn_min,
                              uint64_t dyn_floor) {
  // (the XCD order pads a launch to a multiple of 8 workgroups)
  const bool xcd_order = xcd_swizzle != 0 && cap >= 64;
  if (xcd_order) cap &= ~7ull;
  uint64_t n = want < cap ? want : cap;
  WholeShape s = {};
  // Dynamic tail: the last ~6 % of a launch's tiles (more than twice the 2-3 %
  // by which the XCDs differ), behind a statically mapped part of whole
  // patch rounds; half as many workgroups again as tiles, so that no XCD runs
  // out of workgroups before the tiles run out.
  uint64_t dyn = 0, dyn_wgs = 0;
  if (dyn_min != 0 && xcd_swizzle == 2 && xcd_order && n >= dyn_min && n >= dyn_floor) {
    if (n + n / 8 > cap) n = cap - cap / 8;  // room for the tail's spare workgroups
    const uint64_t fixed = (n - n / 16) / 256 * 256;
    dyn = n - fixed;
    dyn_wgs = dyn + dyn / 2;
    if (fixed + dyn_wgs > cap) dyn = dyn_wgs = 0;  // (tiny block limits: test hook)
  }
  s.tiles = n;
  s.dyn_tiles = (uint32_t)dyn;
  s.dyn_wgs = (uint32_t)dyn_wgs;
  s.launch_tiles = (uint32_t)(n - dyn);
  s.grid = n;
  if (dyn != 0) {  // whole rounds of patches, then the tail
    s.xcd_chunk = 1;
    s.grid = n - dyn + dyn_wgs;
  } else if (xcd_order && n >= 64) {
    if (xcd_swizzle == 2) {  // patches of 32, dealt round-robin to the XCDs
      const uint64_t patches = (n + 31) / 32;
      s.xcd_chunk = 1;
      s.grid = 8ull * 32 * ((patches + 7) / 8);
    } else {
      s.xcd_chunk = (uint32_t)((n + 7) / 8);
      if (s.xcd_chunk == 1) s.xcd_chunk = 2;  // (n >= 64: cannot happen; keeps 1 reserved)
      s.grid = 8ull * s.xcd_chunk;
    }
  }
  return s;
}
// The two kernels' thresholds for the dynamic tail.  Four- and five-product kernels
// (128-sample tiles): the context's threshold, and at least 512 tiles.
constexpr uint64_t kMfmaDynFloor = 512;
// Filter kernel (256-sample tiles): the context's threshold is in 128-sample tiles, a
// quarter of it here; and at least 288 tiles (a static part of 256 and a patch).
constexpr uint64_t kFilterDynFloor = 288;
inline uint64_t filter_dyn_min(uint32_t dyn_tail_tiles) {
  return dyn_tail_tiles == 0 ? 0 : dyn_tail_tiles < 4 ? 1 : dyn_tail_tiles / 4;
}

// Matrix-core kernel, remainder launch (TiledArgs::split_*): split_whole workgroups that
// take one whole tile each, then the pieces -- taken from the counter as well (an XCD that
// finishes its whole tiles early takes more of them): half as many workgroups again.
inline WholeShape split_shape(uint32_t split_whole, uint32_t wgs, uint32_t xcd_swizzle) {
  WholeShape s = {};
  s.tiles = split_whole;
  s.xcd_chunk = xcd_swizzle == 2 && split_whole != 0 && split_whole % 256 == 0;
  s.launch_tiles = split_whole;
  s.dyn_tiles = wgs;
  s.dyn_wgs = wgs + wgs / 2;
  s.grid = (uint64_t)split_whole + s.dyn_wgs;
  return s;
}

// launch_mfma: `first` tiles in whole-tile launches of their own, then (split_tiles != 0)
// ONE launch of split_whole whole tiles and split_tiles tiles cut into pieces.
struct MfmaPlan {
  uint64_t first;
  uint32_t split_whole, split_tiles;
};
// Whole rounds of one tile per workgroup, then the remainder (the tiles that
// would leave most CUs idle for a whole tile time) cut into equal pieces of
// k-steps over all CUs, in the SAME launch: a CU that finishes its last
// whole tile goes straight on to a piece.  For launches of fewer than
// kSplitRounds tiles per CU: 36 tiles 0.57 -> 0.25 ms, 300 tiles
// 1.26 -> 0.91 ms, 820 tiles 2.40 -> 2.15 ms; configs[1] (3160 tiles = 12.3
// rounds, the dispatcher's back-filling does not hide the 13th: time follows
// ceil(rounds), archive/experiments/exp15.sh) 6.93 -> 6.75 ms and 7.12 -> 6.84 ms on two
// boxes.  A piece costs ~30 us per tile it touches (slab, ticket) and the
// pieces end as far apart as the whole tiles before them did (~0.3 ms after
// 12 rounds), which is what is left of the ideal 0.66 x 0.53 ms
// (archive/profiles/r02_tail.txt); beyond 64 rounds the gain is under 1 %.
// wgs: pieces per launch (0 = never split); tile_steps: k-steps of a tile; cap: workgroups
// per launch.
inline MfmaPlan mfma_plan(uint64_t num_tiles, uint32_t wgs, uint32_t tile_steps, uint64_t cap) {
  constexpr uint64_t kSplitRounds = 64;
  uint32_t rest = 0;
  if (wgs != 0 && num_tiles < kSplitRounds * wgs) {
    // under two tiles per CU everything goes out as pieces (300 tiles:
    // 0.98 -> 0.91 ms); otherwise the remainder after whole rounds
    rest = num_tiles < 2ull * wgs ? (uint32_t)num_tiles : (uint32_t)(num_tiles % wgs);
    if ((uint64_t)rest * tile_steps < 8ull * wgs) rest = 0;  // too little work to cut up
  }
  if (rest == 0) return {num_tiles, 0, 0};
  // One launch: `head` whole-tile workgroups followed by the wgs pieces of the
  // remainder, so that CUs finishing their last whole tile go straight on to
  // pieces (a second launch would wait for the slowest whole tile first).
  // Anything beyond one launch's block limit goes out whole before it.
  const uint64_t head = num_tiles - rest;
  uint64_t first = 0;
  if (cap <= wgs + wgs / 2) {
    // (test hook: a block limit below the piece count) whole tiles on their
    // own, in as many launches as it takes, then the pieces
    first = head;
  } else if (head + wgs + wgs / 2 > cap) {  // (the pieces' launch has wgs / 2 spare workgroups)
    first = head + wgs + wgs / 2 - cap;
  }
  return {first, (uint32_t)(head - first), rest};
}

// launch_filter, one launch chunk: n tiles, of which the last `rest` are cut into `parts`
// pieces of k each (workgroups fsplit_first .. grid - 1, TiledArgs::fsplit_*) behind the
// whole-tile part; check0 / check1 / rotate as the kernel reads them.
struct FilterPlan {
  uint64_t n;
  uint32_t check0, check1, rotate;
  uint32_t rest, parts;
  WholeShape whole;
  uint32_t fsplit_tile0, fsplit_first;
  uint64_t grid;
};
// want: tiles left; cap: tiles per chunk; wgs: one per CU; tile_steps: k-steps of 256 sites;
// checks: the workspace has check points' flags; can_split: and slabs for remainder pieces;
// max_slabs: kFilterSplitSlabs.
inline FilterPlan filter_plan(uint64_t want, uint64_t cap, uint32_t wgs, uint32_t tile_steps,
                              bool checks, bool can_split, uint32_t max_slabs,
                              const LaunchSwitches &sw) {
  FilterPlan p = {};
  const uint64_t n = want < cap ? want : cap;
  p.n = n;
  // check 0 (the forecast): for launches of fewer than 16 rounds, where the tiles that
  // would have to give up make up most of the launch before anybody has finished
  p.check0 = !checks ? 0u : sw.check0 == 2 ? 2u : (sw.check0 == 1 && n < 16ull * wgs) ? 1u : 0u;
  // (bits 8-15: check_emit; bit 16: the forecast's switch, whatever the launch's length)
  p.check1 = checks ? sw.check1 | (sw.check_emit << 8) | (sw.check0 != 0 ? 1u << 16 : 0u) : 0u;
  // (rotated tiles: for launches of many rounds -- the tiles of a few rounds have not
  //  drifted apart yet, configs[1] has an L2 hit rate of 0.76 without)
  p.rotate = checks && (n >= sw.rotate_min_tiles || sw.rotate >= 2) ? sw.rotate : 0u;
  // Short launches: the tiles beyond whole rounds of one per CU would leave most
  // CUs idle for a whole tile time; each of them is cut into `parts` pieces of k
  // instead (same launch, behind the whole tiles).
  uint32_t rest = 0, parts = 0;
  if (can_split && n < 16ull * wgs) {
    rest = (uint32_t)(n % wgs);
    if (rest != 0 && 2 * rest <= wgs && rest <= max_slabs / 2) {
      parts = wgs / rest;
      if (parts > 8) parts = 8;
      if (parts * rest > max_slabs) parts = max_slabs / rest;
      // (pieces of at least 8 k-steps, unless a test says otherwise: the pipeline's fill
      //  and the slab are per piece)
      const uint32_t min_steps = sw.split_min_steps != 0 ? sw.split_min_steps : 8;
      while (parts > 1 && tile_steps / parts < min_steps) --parts;
    }
    if (parts < 2) rest = parts = 0;
  }
  p.rest = rest;
  p.parts = parts;
  // the tiles that go out whole: patches or nothing (no chunk form), one launch
  p.whole = whole_shape(n - rest, ~0ull, sw.xcd_swizzle == 2 ? 2u : 0u,
                        filter_dyn_min(sw.dyn_tail_tiles), kFilterDynFloor);
  // ... and behind them the pieces of the remainder
  p.fsplit_tile0 = (uint32_t)(n - rest);
  p.fsplit_first = (uint32_t)p.whole.grid;
  p.grid = p.whole.grid + (uint64_t)rest * parts;
  return p;
}

}  // namespace cuking

#endif  // CUKING_AMD_KING_LAUNCH_PLAN_H_
