// C ABI of the KING hot path (include/cuking_amd.h): context, device memory,
// layout preparation + kernel launch, timing hooks.  gfx950 only; no CPU
// fallback -- every device entry point fails with CUKING_ERR_DEVICE when HIP
// cannot provide a gfx950 device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "king_common.h"
#include "king_geno.h"
#include "king_host.h"
#include "king_ibd.h"
#include "king_kin_summary.h"
#include "king_ld.h"
#include "king_site_qc.h"
#include "king_unrelated.h"

using namespace cuking;

namespace {

#define HIP_TRY(expr)                                                      \
  do {                                                                     \
    const hipError_t _e = (expr);                                          \
    if (_e != hipSuccess) {                                                \
      (void)hipGetLastError(); /* do not leave it sticky for other users */ \
      return cuking_fail(_e == hipErrorOutOfMemory ? CUKING_ERR_OUT_OF_MEMORY     \
                                            : CUKING_ERR_DEVICE,           \
                  "%s failed: %s", #expr, hipGetErrorString(_e));          \
    }                                                                      \
  } while (0)

// Makes the context's device current, or returns bind()'s refusal.
#define BIND_OR_RETURN(ctx)                    \
  do {                                         \
    const cuking_status _st = bind(ctx);       \
    if (_st != CUKING_OK) return _st;          \
  } while (0)

uint32_t ceil_div(uint32_t a, uint32_t b) {
  return (uint32_t)(((uint64_t)a + b - 1) / b);
}
uint32_t round_up(uint32_t a, uint32_t b) { return ceil_div(a, b) * b; }

struct EventPair {
  hipEvent_t start = nullptr, stop = nullptr;
};

struct Timer {
  std::vector<EventPair> pool;
  size_t used = 0;

  hipError_t begin(hipStream_t s, EventPair **out) {
    if (used == pool.size()) {
      EventPair p;
      hipError_t e = hipEventCreate(&p.start);
      if (e != hipSuccess) return e;
      e = hipEventCreate(&p.stop);
      if (e != hipSuccess) return e;
      pool.push_back(p);
    }
    *out = &pool[used++];
    return hipEventRecord((*out)->start, s);
  }
  hipError_t collect(double *ms, uint64_t *n) {
    *ms = 0;
    *n = used;
    for (size_t k = 0; k < used; ++k) {
      hipError_t e = hipEventSynchronize(pool[k].stop);
      if (e != hipSuccess) return e;
      float t = 0;
      e = hipEventElapsedTime(&t, pool[k].start, pool[k].stop);
      if (e != hipSuccess) return e;
      *ms += t;
    }
    return hipSuccess;
  }
  void destroy() {
    for (auto &p : pool) {
      if (p.start) (void)hipEventDestroy(p.start);
      if (p.stop) (void)hipEventDestroy(p.stop);
    }
    pool.clear();
    used = 0;
  }
};

}  // namespace

struct cuking_ctx {
  int device = 0;
  cuking_kernel kernel = CUKING_KERNEL_TILED;
  int variant = 0;
  // Tile rows per scheduling band.  NOT a multiple of 8: workgroups are dealt
  // round-robin over the 8 XCDs, so with 16 rows per band every XCD would see
  // the same rows in every column -- and rows differ in how many of their
  // tiles are real (triangle, strided rectangles): measured 6.7 ms vs 4.3 ms
  // for a rank's strided launch (tools/rect_probe.py).
  // 0 = by block size (band_rows_for below); tests and tuning runs pin a value.
  uint32_t band_rows = 0;
  int counts_mode = -1;  // -1 auto, 0 lean (4 sums + recount), 1 full (5 sums)
  int xcd_swizzle = 2;   // matrix-core kernel: XCD-aware order, 0 off / 1 chunks / 2 patches (king_common.h)
  uint32_t dyn_tail_tiles = 16384;  // launches of at least this many tiles get a dynamic tail; 0 = never

  // Workspace of the tiled kernel: the k-major planes and the band prefix.
  uint4 *planes = nullptr;
  size_t planes_bytes = 0;
  uint64_t *band_prefix = nullptr;
  size_t band_prefix_bytes = 0;
  TileSpace prefix_for = {0, 0, 0, 0};  // tile space the prefix was built for

  // Remainder splitting of the matrix-core kernel (king_mfma.hip): split_wgs
  // workgroups = one per CU.  0 = never split.
  uint32_t split_wgs = 0;
  uint32_t num_cus = 0;  // what cuking_unrelated_set sizes its grids from
  // Scratch of one stream that launches pair kernels (launches on different streams may
  // overlap): the matrix-core kernel's zeroed remainder slab, and the filter variant's
  // control words, candidate list, dense-quadrant list and slabs (king_filter.hip), sized
  // for a block of `filter_tiles` tiles (of its enumeration).  Each is allocated on first
  // use; at most kMaxStreams streams, the oldest makes room (stream_entry below).
  struct DeviceBuf {
    void *p = nullptr;
    size_t bytes = 0;
  };
  struct StreamScratch {
    hipStream_t stream;
    uint32_t *split = nullptr;
    uint8_t *filter = nullptr;
    uint64_t filter_tiles = 0;
    // Grown when a call needs more (grow_on_stream below): cuking_unrelated_set's workspace
    // (king_prune.hip), cuking_compact_sites' table (king_site_qc.h) and the record counter of
    // cuking_ld_edges and cuking_pcrelate_records (one word; each call zeroes it on the stream
    // and has read it back when it returns; cuking_ibd_pairs counts its segments there too),
    // and the group-start bitmask of cuking_ibd_pairs (king_ibd.h; each call rebuilds it on
    // the stream).
    // ... and the site order's scratch (king_sort.hip: counts, the sort, the permuted bitset;
    // each conversion with the order on rebuilds it on the stream).
    DeviceBuf prune, sites, record_count, ibd_groups, site_order;
  };
  std::vector<StreamScratch> scratch;
  // The running totals of filter scratch that has been freed since (a larger block took
  // its place, its stream made room): the diagnostics count over the context's life.
  unsigned long long filter_totals_retired[kNumTotals] = {};
  // (the two caps are options so that tests can force the dense and the list-full paths)
  uint32_t filter_quadrant_cap = kFilterQuadrantCap;
  uint32_t filter_cand_cap = kFilterCandCap;
  uint32_t filter_split_min_steps = 8;  // k-steps per remainder piece, at least
  // Check points of the filter kernel (king_common.h): check 0 (forecast) 0 off, 1 for
  // launches of fewer than 16 rounds, 2 always; check 1 (rigorous) 0 off, 1 the entry the
  // kernel picks from threshold and cohort, 2 + k entry k of the share menu forced.
  int filter_check0 = 1, filter_check1 = 1, filter_check_emit = (int)kCheckEmitCap;
  // Rotated tiles (king_common.h TiledArgs::rotate): 0 off, 1 on, 2 / 3 + j test hooks;
  // bitsets of fewer k-steps (of 256 sites) than the minimum are not rotated.
  int filter_rotate = 1;
  uint32_t filter_rotate_min_steps = 128;
  uint32_t filter_rotate_min_tiles = 2048;  // 8 rounds of one tile per CU
  // The kernel layout's samples sorted by their share of missing calls (king_sort.hip);
  // the four-product kernel's codes converted only when the filter needs them
  // (0: with every conversion).
  // filter_sort: 0 never; 1 (default) whole-block conversions -- cuking_compute_king and
  // cuking_compute_king_tiles, whose tiles are opaque units of work; 2 also the ranges of
  // cuking_prepare_samples (for hosts whose rectangles cover every prepared range in full
  // or in a union, like the staged multi-GPU schedules: inside a sorted range the samples
  // behind a sub-rectangle are not the ones its bounds name).
  int filter_sort = 1;
  bool filter_lazy_codes = true;
  // The kernel layout's SITES in the order of the X they contribute to unrelated pairs
  // (king_sort.hip "Site order"): -1 (default) for whole-block conversions of calls the filter
  // runs for, on blocks of at least kSiteOrderMinTiles tiles with check points, whose curve
  // forecasts a check at least kSiteOrderMinGain 64ths earlier than stored order's at the
  // call's threshold (prepare() reads the curve back: one host wait per such conversion); 0
  // never; 1 for every such conversion whatever the block's size and the forecast.  Bitsets
  // too wide for the gather (site_order_scratch) keep stored order; so do the ranges of a
  // staged pass.
  int filter_site_order = -1;
  uint32_t filter_site_order_min_tiles = (uint32_t)kSiteOrderMinTiles;  // (test hook)
  // The kernel that writes the ordered copy (site_gather_pick): -1 (default) 4 samples per
  // LDS field where the sites fit, else 2, else the ballot kernel; 0 the ballot kernel; 4 / 2
  // forced (4 is refused by the conversion where it does not fit).  Same bytes either way.
  int filter_site_gather = -1;
  // What the last conversion that built a curve read from it (read-only keys
  // "site_order_share", "site_order_stored_share", "site_order_sigma_e6", "site_order_on").
  SiteOrderForecast order_forecast = {0, 0, false};
  float order_sigma = 0.f;
  void *sort_temp = nullptr;
  size_t sort_temp_bytes = 0;

  // The synthetic generator's per-site and per-sample tables (synth.hip), and an event
  // behind the last launch that reads them: a call on another stream waits for it before
  // it rewrites them.
  void *synth_tables = nullptr;
  size_t synth_tables_bytes = 0;
  hipStream_t synth_stream = nullptr;
  hipEvent_t synth_done = nullptr;

  // What the plane workspace holds: the block it was converted for and which
  // 64-sample plane tiles of it have been converted (cuking_compute_king_rect
  // refuses to read anything else).
  struct Prepared {
    bool valid = false;
    cuking_submatrix sm = {0, 0, 0, 0};
    uint32_t words_per_sample = 0;
    int variant = -1;
    uint32_t tile = 0;  // tile edge of the geometry (the context variant's)
    const uint64_t *bits = nullptr;
    bool codes = true;  // every converted tile has its nibble codes (false: T2 only, lazy)
    // converted for a dense kinship matrix: never sorted, whatever "filter_sort" says (a
    // call of the other kind does not take the layout over: it converts again)
    bool dense_order = false;
    // the T2 layout and the per-sample counts hold the sites in the site order, and the
    // workspace its curve (TiledArgs::site_curve); order_wanted: the conversion was one the
    // option let build a curve (site_order: ... and the curve said yes, or the option was 1)
    bool site_order = false, order_wanted = false;
    // the threshold of the call the order was decided for, and -- after an automatic "no" --
    // the conversions of this block at that threshold that still trust it without building
    // the curve again (kSiteOrderNoTrust: the bitset behind the pointer may have changed, but
    // a stale "no" only costs what stored order costs)
    float order_thr = 0.f;
    uint32_t order_no_left = 0;
    // per 64 plane samples: 0 = not converted, 1 = converted (kernels that
    // read it, if any, all precede the tail of `ordered_on`), 2 = converted
    // and read by kernels enqueued since
    std::vector<uint8_t> tiles;
    hipStream_t ordered_on = nullptr;
    bool ordered_valid = false;
  } prepared;
  // Streams with pair kernels that may still be reading the workspace, each
  // with an event to order a later rewrite after them.
  std::vector<std::pair<hipStream_t, hipEvent_t>> readers;

  // Hosts that promise not to rewrite a bitset in place without telling
  // (cuking_invalidate) may skip the conversion when the workspace already
  // holds this block ("reuse_prepared"); off by default: like the reference's
  // kernel, a call then reads whatever the bitset holds when it runs.
  bool reuse_prepared = false;
  // Book-keeping for hosts that must not allocate or synchronise while
  // collectives of other devices are in flight (cuking_ctx_reserve): device
  // allocations made for the workspace, and host-side waits, so far.
  uint64_t workspace_allocations = 0, host_syncs = 0, conversions_skipped = 0;

  bool timing = false;
  Timer king_timer, prepare_timer;
};

namespace {

int default_variant() {
  if (const char *v = getenv("CUKING_AMD_VARIANT")) {
    const int k = atoi(v);
    if (k >= 0 && k < kNumTiledVariants) return k;
  }
  return kMfmaFilterVariant;
}

// The variant that runs for a bitset of this width: the matrix-core variant
// counts in float32 (exact below 2^24 sites); wider bitsets take the VALU
// variant with the same tile edge and k padding, so tile indices, tile bounds
// and prepared ranges mean the same either way.
int effective_variant(const cuking_ctx *ctx, uint32_t words_per_sample) {
  const uint64_t sites = (uint64_t)round_up(words_per_sample, 8) * 32;
  int v = ctx->variant;
  // (the four-product variant decides on an integer that matches the
  //  reference's float expression below 2^22 sites only)
  if ((v == kMfmaN4Variant || v == kMfmaFilterVariant) && sites > kMfmaN4MaxSites) v = kMfmaVariant;
  if (v == kMfmaVariant && sites > kMfmaMaxSites) v = 2;
  return v;
}

// The shape everything about a call is laid out for: the kernel variant that
// runs (layout, k padding) with the tile edge of the CONTEXT's variant, so that
// tile indices, tile bounds and prepared ranges never depend on the width of
// the bitset.  When the two differ (filter variant, 256-sample tiles, falling
// back to a 128-tile kernel for a wide bitset) the kernel runs in quadrant mode.
TiledVariant plan_variant(const cuking_ctx *ctx, uint32_t words_per_sample) {
  TiledVariant v = tiled_variant(effective_variant(ctx, words_per_sample));
  v.tile = tiled_variant(ctx->variant).tile;
  return v;
}

// Which form of the tiled kernel.  The lean form keeps four sums per pair but
// recounts hom/hom sites for every EMITTED pair; the full form keeps five sums
// for every pair.  Measured at 10k x 100k sites: VALU kernels lean 27.8 ms +
// 3 ms per 10^6 emitted pairs against full 34.4 ms flat; matrix-core kernel
// lean 7.0 ms + 10 ms per 10^6 emitted pairs against full 8.8 ms + 0.9 ms per
// 10^6 (the fifth sum in a pass of its own, king_mfma.hip).  For unrelated
// samples kinship scatters around 0 with a spread ~ 1/sqrt(sites) (at 100k
// sites 2 % of the pairs exceed 0.005, 0.3 % exceed 0.007), so the automatic
// choice is lean iff kin_threshold > c / sqrt(sites) with c = 1.6 (VALU) or
// 2.05 (matrix cores: break-even near 0.4 % of the pairs emitted).  Either
// form gives the same records.
bool use_full_counts(const cuking_ctx *ctx, float kin_threshold, uint32_t words_per_sample) {
  if (ctx->counts_mode == 1) return true;
  if (ctx->counts_mode == 0) return false;
  if (!(kin_threshold > 0.0f)) return true;
  const double sites = 32.0 * words_per_sample;
  const double c = is_mfma_variant(effective_variant(ctx, words_per_sample)) ? 2.05 : 1.6;
  return (double)kin_threshold * kin_threshold * sites < c * c;
}

cuking_status bind(cuking_ctx *ctx) {
  if (ctx == nullptr) return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null context");
  HIP_TRY(hipSetDevice(ctx->device));
  return CUKING_OK;
}

PlaneGeometry make_geometry(const cuking_submatrix &sm,
                            uint32_t words_per_sample,
                            const TiledVariant &v) {
  PlaneGeometry g;
  g.num_rows = sm_num_rows(sm);
  g.num_cols = sm_num_cols(sm);
  g.diag = sm_is_diag(sm) ? 1u : 0u;
  g.rows_padded = round_up(g.num_rows, v.tile);
  g.cols_padded = round_up(g.num_cols, v.tile);
  g.col_base = g.diag ? 0u : g.rows_padded;
  g.s_stride = g.diag ? g.rows_padded : g.rows_padded + g.cols_padded;
  g.k_words = round_up(words_per_sample, v.k_chunk);  // 2 x 32-bit per u64 / 2 planes
  return g;
}

// Band height when the caller has not pinned one.  Measured on MI355X with the
// XCD-aware order (archive/profiles/r02_xcd_order.txt): the matrix-core kernel wants
// the 32 tiles an XCD holds at a time to be a compact patch, 5 rows x ~6
// columns (11 strips through one L2 instead of 32): 100k x 100k 645 -> 621 ms,
// 300k x 150k 9.33 -> 8.69 s.  Below ~128 tile rows the bitset sits in the
// Infinity Cache anyway and 17 rows measured 2-3 % better (10k samples:
// 7.04 -> 6.77 ms with the XCD order, 6.96 with 5 rows).  The VALU kernels
// keep 17 (see cuking_ctx::band_rows in the round-1 notes, tools/rect_probe.py).
uint32_t band_rows_for(uint32_t pinned, const PlaneGeometry &g, const TiledVariant &v) {
  if (pinned != 0) return pinned;
  if (v.layout == kLayoutWord) return 17;
  // 256-sample tiles (filter variant): 8 rows x 4 columns per XCD patch at every size
  // (configs[2]: 146.8 ms against 147.4 with 5 rows and 147.2 with 17; configs[1]: 1.78
  // against 1.81 with 17; profiles/r03_ablation.txt)
  if (v.tile == kFilterTile) return 8;
  return g.rows_padded / v.tile >= 128 ? 5 : 17;
}

TileSpace make_tiles(const PlaneGeometry &g, const TiledVariant &v,
                     uint32_t band_rows) {
  band_rows = band_rows_for(band_rows, g, v);
  TileSpace t;
  t.tiles_r = g.rows_padded / v.tile;
  t.tiles_c = g.cols_padded / v.tile;
  t.band_rows = band_rows;
  t.diag = g.diag;
  return t;
}

uint64_t total_tiles(const TileSpace &t) {
  uint64_t n = 0;
  for (uint32_t b = 0; b < t.num_bands(); ++b) n += t.band_tiles(b);
  return n;
}

// Streams whose scratch a context keeps (torch hands out new stream handles: the cache
// stays small).
constexpr size_t kMaxStreams = 8;

// Frees the filter scratch of a stream on which nothing runs any more; with `retire` its
// running totals join the context's.
void free_filter_scratch(cuking_ctx *ctx, cuking_ctx::StreamScratch &e, bool retire = true) {
  if (e.filter == nullptr) return;
  unsigned long long v[kNumTotals] = {};
  if (retire) {
    if (hipMemcpy(v, e.filter + filter_scratch_layout(e.filter_tiles).totals, sizeof v,
                  hipMemcpyDeviceToHost) == hipSuccess)
      for (uint32_t k = 0; k < kNumTotals; ++k) ctx->filter_totals_retired[k] += v[k];
    (void)hipGetLastError();
  }
  (void)hipFree(e.filter);
  e.filter = nullptr;
}

void free_split_slab(cuking_ctx::StreamScratch &e) {
  if (e.split != nullptr) (void)hipFree(e.split);
  e.split = nullptr;
}

// Frees everything an entry of the stream cache owns, once nothing runs on its stream any
// more: THE list of its buffers (a new one is added to StreamScratch and here).
void free_stream_scratch(cuking_ctx *ctx, cuking_ctx::StreamScratch &e, bool retire_totals) {
  free_filter_scratch(ctx, e, retire_totals);
  free_split_slab(e);
  for (cuking_ctx::DeviceBuf *b :
       {&e.prune, &e.sites, &e.record_count, &e.ibd_groups, &e.site_order}) {
    if (b->p != nullptr) (void)hipFree(b->p);
    *b = {};
  }
}

// Waits for the stream of ctx->scratch[k] and drops its entry.  A stream its owner has
// destroyed meanwhile cannot be waited for, but work it held may still run: then the
// whole device is waited for.
void evict_scratch(cuking_ctx *ctx, size_t k) {
  cuking_ctx::StreamScratch &e = ctx->scratch[k];
  ++ctx->host_syncs;
  if (hipStreamSynchronize(e.stream) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipDeviceSynchronize();
    (void)hipGetLastError();
  }
  free_stream_scratch(ctx, e, true);
  ctx->scratch.erase(ctx->scratch.begin() + (ptrdiff_t)k);
}

// The entry of `stream` in the context's cache, created (empty: no allocation) when the
// stream has none, after the oldest entry has made room when the cache is full.  The pointer
// is valid until the next call that may add or drop an entry: stream_entry and evict_scratch.
cuking_ctx::StreamScratch *stream_entry(cuking_ctx *ctx, hipStream_t stream) {
  for (auto &x : ctx->scratch)
    if (x.stream == stream) return &x;
  if (ctx->scratch.size() >= kMaxStreams) evict_scratch(ctx, 0);
  ctx->scratch.push_back({stream});
  return &ctx->scratch.back();
}

// Makes the stream-owned buffer *buf at least `need` bytes.  Replacing one waits for its
// stream first (an earlier call on it may still use the old one) and leaves the entry clean
// should the allocation fail.
cuking_status grow_on_stream(cuking_ctx *ctx, hipStream_t stream, cuking_ctx::DeviceBuf *buf,
                             size_t need) {
  if (need <= buf->bytes) return CUKING_OK;
  if (buf->p != nullptr) {
    ++ctx->host_syncs;
    HIP_TRY(hipStreamSynchronize(stream));
    (void)hipFree(buf->p);
    *buf = {};
  }
  HIP_TRY(hipMalloc(&buf->p, need));
  ++ctx->workspace_allocations;
  buf->bytes = need;
  return CUKING_OK;
}

// THE counted output: `launch(d_count, stream)` writes up to `max` items and counts all of them
// into the zeroed count word of the stream's scratch; the count is read back (one host sync)
// into *num and judged by `count_status(count, max)`: RESOURCE_EXHAUSTED with the exact count
// when they do not fit.
template <class Launch>
cuking_status counted_output(cuking_ctx *ctx, hipStream_t s, uint64_t max, uint64_t *num,
                             cuking_status (*count_status)(uint64_t, uint64_t), Launch &&launch) {
  cuking_ctx::StreamScratch *e = stream_entry(ctx, s);
  const cuking_status st = grow_on_stream(ctx, s, &e->record_count, sizeof(unsigned long long));
  if (st != CUKING_OK) return st;
  unsigned long long *d_count = static_cast<unsigned long long *>(e->record_count.p);
  HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), s));
  HIP_TRY(launch(d_count, s));
  unsigned long long count = 0;
  HIP_TRY(hipMemcpyAsync(&count, d_count, sizeof(count), hipMemcpyDeviceToHost, s));
  ++ctx->host_syncs;
  HIP_TRY(hipStreamSynchronize(s));
  *num = count;
  return count_status(count, max);
}

// What a launch of the context's variant needs per stream.
bool uses_split_slab(const cuking_ctx *ctx) {
  return ctx->split_wgs != 0 && is_mfma_variant(ctx->variant);
}
bool uses_filter_scratch(const cuking_ctx *ctx) { return ctx->variant == kMfmaFilterVariant; }

// A device buffer of `bytes` whose bytes [zero_at, zero_at + zero_bytes) read zero when
// the first kernel on `stream` starts: zeroed ON that stream (a null-stream memset is not
// ordered against a non-blocking stream, and fresh memory holds whatever was there before).
cuking_status alloc_scratch(cuking_ctx *ctx, void **p, size_t bytes, size_t zero_at,
                            size_t zero_bytes, hipStream_t stream) {
  HIP_TRY(hipMalloc(p, bytes));
  ++ctx->workspace_allocations;
  const hipError_t e = hipMemsetAsync(static_cast<uint8_t *>(*p) + zero_at, 0, zero_bytes, stream);
  if (e != hipSuccess) {
    (void)hipFree(*p);
    *p = nullptr;
    HIP_TRY(e);
  }
  return CUKING_OK;
}

// The scratch of `stream` for a block of `tiles` tiles (of its enumeration), allocated on
// first use -- the filter scratch again when a larger block comes --, or nullptr when the
// context's variant needs none.
cuking_status scratch_for(cuking_ctx *ctx, hipStream_t stream, uint64_t tiles,
                          cuking_ctx::StreamScratch **out) {
  *out = nullptr;
  const bool split = uses_split_slab(ctx), filter = uses_filter_scratch(ctx);
  if (!split && !filter) return CUKING_OK;
  cuking_ctx::StreamScratch *e = stream_entry(ctx, stream);
  cuking_status st;
  if (split && e->split == nullptr) {
    // (the tickets in front of the slab)
    st = alloc_scratch(ctx, reinterpret_cast<void **>(&e->split),
                       mfma_split_scratch_bytes(ctx->split_wgs), 0,
                       mfma_split_counter_bytes(ctx->split_wgs), stream);
    if (st != CUKING_OK) return st;
  }
  const FilterScratchLayout want = filter_scratch_layout(tiles);
  if (filter && e->filter != nullptr && filter_scratch_layout(e->filter_tiles).bytes < want.bytes) {
    // a larger block: kernels of this stream may still use the old lists
    ++ctx->host_syncs;
    HIP_TRY(hipStreamSynchronize(stream));
    free_filter_scratch(ctx, *e);
  }
  if (filter && e->filter == nullptr) {
    // (the running totals behind "filter_candidates" / "filter_dense_quadrants" and the
    //  tickets of the remainder pieces, zero between launches)
    st = alloc_scratch(ctx, reinterpret_cast<void **>(&e->filter), want.bytes, want.totals,
                       kFilterCtrlBytes + kFilterTicketBytes, stream);
    if (st != CUKING_OK) return st;
    e->filter_tiles = tiles;
  }
  *out = e;
  return CUKING_OK;
}

// The filter's bound applies to a call (it only helps the lean form with a threshold inside
// (0, 1/2)): the filter kernel runs (LaunchSwitches::filter_runs), and the four-product
// kernel's codes may stay unconverted.
bool filter_runs(const cuking_ctx *ctx, uint32_t words_per_sample, CallForm form, bool full,
                 float kin_threshold) {
  return kCallForms[form].filter_may_run &&
         effective_variant(ctx, words_per_sample) == kMfmaFilterVariant && !full &&
         kin_threshold > 0.f && kin_threshold < 0.5f;
}

// The context's switches for a call of `form` that runs the `full` or the lean k loop: built
// once per call, in front of the conversion (which asks whether the filter runs).
LaunchSwitches launch_switches(const cuking_ctx *ctx, uint32_t words_per_sample, CallForm form,
                               bool full, float kin_threshold) {
  LaunchSwitches sw;
  sw.xcd_swizzle = (uint32_t)ctx->xcd_swizzle;
  sw.dyn_tail_tiles = ctx->dyn_tail_tiles;
  sw.check0 = (uint32_t)ctx->filter_check0;
  sw.check1 = (uint32_t)ctx->filter_check1;
  sw.check_emit = (uint32_t)ctx->filter_check_emit;
  sw.rotate = (uint32_t)ctx->filter_rotate;
  sw.rotate_min_tiles = ctx->filter_rotate_min_tiles;
  sw.split_min_steps = ctx->filter_split_min_steps;
  sw.filter_runs = filter_runs(ctx, words_per_sample, form, full, kin_threshold);
  sw.form = form;
  return sw;
}

// What a pair call produces: its form (king_launch_plan.h), named by the entry point, the
// threshold it runs at, and the outputs of that form (the others stay null).
struct Outputs {
  CallForm form;
  // records: the call's; relative counts: rel_thr[0] (the filter's bound, the layout and the
  // lean form's cheap test all follow the lowest threshold); every other form: 0
  float kin_threshold;
  uint32_t max_results;
  cuking_result *results;
  uint32_t *result_index, *result_overflow;
  cuking_counts *counts;
  // dense kinship matrix (TiledArgs::dense_kin): every pair's float32 kinship, no records
  float *kin;
  uint64_t kin_ld;
  uint32_t kin_flags;
  // kinship summary (TiledArgs::sum_hist / sum_best): every pair's kinship reduced, no records
  uint64_t *sum_hist, *sum_best;
  cuking_kin_bins sum_bins;
  // relative counts (TiledArgs::rel_counts): the thresholded call without records
  uint32_t *rel_counts;
  uint32_t rel_num;
  float rel_thr[CUKING_REL_THRESHOLDS_MAX];
  // PI_HAT records (TiledArgs::pihat): the full form with the PI_HAT decision
  PihatArgs pihat;
};
// A records call's, or with a PI_HAT decision a PI_HAT call's.
Outputs record_outputs(CallForm form, float kin_threshold, uint32_t max_results,
                       cuking_result *results, uint32_t *result_index,
                       uint32_t *result_overflow) {
  Outputs out = {};
  out.form = form;
  out.kin_threshold = kin_threshold;
  out.max_results = max_results;
  out.results = results;
  out.result_index = result_index;
  out.result_overflow = result_overflow;
  return out;
}
// The device arguments of the pair kernels for the block `sm` of the prepared workspace
// (geometry `geo`, enumeration `tiles`; the stream's filter scratch sized for
// `block_tiles`).  Callers fill in the tile range.
cuking_status launch_args(cuking_ctx *ctx, hipStream_t stream, const cuking_submatrix &sm,
                          uint32_t words_per_sample, const uint64_t *d_bit_sets,
                          const PlaneGeometry &geo, const TileSpace &tiles,
                          uint64_t block_tiles, const Outputs &out, TiledArgs *args) {
  TiledArgs &a = *args;
  a = {};
  a.planes = ctx->planes;
  a.geo = geo;
  a.tiles = tiles;
  a.band_prefix = ctx->band_prefix;
  a.i_begin = sm.i_begin;
  a.j_begin = sm.j_begin;
  a.kin_threshold = out.kin_threshold;
  a.max_results = out.max_results;
  a.results = out.results;
  a.result_index = out.result_index;
  a.result_overflow = out.result_overflow;
  a.dense_counts = out.counts;
  a.dense_kin = out.kin;
  a.kin_ld = out.kin_ld;
  a.kin_diag = (out.kin != nullptr && (out.kin_flags & CUKING_KIN_SYMMETRIC)) ? 1u : 0u;
  a.sum_hist = reinterpret_cast<unsigned long long *>(out.sum_hist);
  a.sum_best = reinterpret_cast<unsigned long long *>(out.sum_best);
  if (out.sum_hist != nullptr) {
    a.sum_lo = out.sum_bins.lo;
    a.sum_scale = kin_bin_scale(out.sum_bins);  // (once per call, on the host)
    a.sum_bins = out.sum_bins.num_bins;
  }
  a.rel_counts = out.rel_counts;
  if (out.rel_counts != nullptr) {
    a.rel_num = out.rel_num;
    for (uint32_t t = 0; t < out.rel_num; ++t) a.rel_thr[t] = out.rel_thr[t];
  }
  a.pihat = out.pihat;
  a.rect_row_stride = 1;
  a.bits = d_bit_sets;
  a.words_per_sample = words_per_sample;
  a.split_wgs = ctx->split_wgs;
  // the sample order of the workspace's layout (none where the form's conversion did not
  // sort: the identity), and the lazy-codes word
  if (plan_variant(ctx, words_per_sample).layout == kLayoutNibbleStats) {
    if (!kCallForms[out.form].unsorted) a.perm = plane_perm(ctx->planes, geo);
    if (!ctx->prepared.codes) a.codes_ready = plane_flags(ctx->planes, geo);
  }
  cuking_ctx::StreamScratch *e;
  const cuking_status st = scratch_for(ctx, stream, block_tiles, &e);
  if (st != CUKING_OK || e == nullptr) return st;
  if (uses_split_slab(ctx)) {
    a.split_counters = e->split;
    a.split_scratch = e->split + mfma_split_counter_bytes(ctx->split_wgs) / sizeof(uint32_t);
  }
  if (!uses_filter_scratch(ctx)) return CUKING_OK;
  uint8_t *base = e->filter;
  const FilterScratchLayout l = filter_scratch_layout(e->filter_tiles);
  a.sample_stats = plane_stats(ctx->planes, geo);
  a.t2 = plane_t2(ctx->planes, geo);
  a.prefix_u = plane_prefix_u(ctx->planes, geo);
  a.cohort_sums = plane_cohort_sums(ctx->planes, geo);
  a.filter_ctrl = reinterpret_cast<uint32_t *>(base);
  a.filter_totals = reinterpret_cast<unsigned long long *>(base + l.totals);
  a.fsplit_tickets = reinterpret_cast<uint32_t *>(base + l.tickets);
  a.tile_done = base + l.tile_done;
  a.cand_list = reinterpret_cast<uint2 *>(base + l.cand);
  a.cand_cap = ctx->filter_cand_cap < l.cand_entries ? ctx->filter_cand_cap : l.cand_entries;
  a.quadrant_cap = ctx->filter_quadrant_cap;
  a.dense_list = reinterpret_cast<uint2 *>(base + l.dense);
  a.dense_cap = l.chunk_tiles * 4;
  // (remainder splitting follows the matrix-core kernels' switch: "split_wgs" 0 = never)
  a.fsplit_slabs = ctx->split_wgs != 0 ? reinterpret_cast<float4 *>(base + l.slabs) : nullptr;
  a.rotate_min_steps = ctx->filter_rotate_min_steps;
  a.check_steps = plane_check_steps(ctx->planes, geo);
  if (ctx->prepared.site_order) a.site_curve = plane_site_curve(ctx->planes, geo);
  a.site_lap = ctx->filter_site_order == 2 || (ctx->filter_site_order == -1 && kSiteOrderAutoLap);
  return CUKING_OK;
}

// Enqueues `num_tiles` tiles of the planned geometry with the kernel variant that runs for
// this width of bitset.
hipError_t launch_planned(const cuking_ctx *ctx, uint32_t words_per_sample, bool full,
                          const TiledArgs &a, const LaunchSwitches &sw, uint64_t num_tiles,
                          hipStream_t stream) {
  return launch_tiled(effective_variant(ctx, words_per_sample), tiled_variant(ctx->variant).tile,
                      full, a, sw, num_tiles, stream);
}

// A pair kernel that reads the workspace has been enqueued on `stream`.
void note_reader(cuking_ctx *ctx, hipStream_t stream) {
  for (auto &r : ctx->readers)
    if (r.first == stream) return;
  ctx->readers.emplace_back(stream, nullptr);
}

// Orders `stream` behind every pair kernel enqueued so far on OTHER streams
// (same-stream work is ordered anyway): the caller is about to rewrite plane
// data they may still read.  One context serves one host thread at a time, so
// "enqueued so far" is everything there is.  Afterwards the tail of `stream`
// stands for all of them (it stays in the list as their proxy), and no plane
// tile counts as "being read" any more.
cuking_status wait_for_readers(cuking_ctx *ctx, hipStream_t stream) {
  bool failed = false;
  for (auto &r : ctx->readers) {
    if (r.first == stream) continue;
    if (r.second == nullptr &&
        hipEventCreateWithFlags(&r.second, hipEventDisableTiming) != hipSuccess) {
      failed = true;
      break;
    }
    if (hipEventRecord(r.second, r.first) != hipSuccess ||
        hipStreamWaitEvent(stream, r.second, 0) != hipSuccess) {
      failed = true;  // e.g. a stream the caller has destroyed meanwhile
      break;
    }
  }
  if (failed) {
    (void)hipGetLastError();
    ++ctx->host_syncs;
    HIP_TRY(hipDeviceSynchronize());
  }
  for (auto &r : ctx->readers)
    if (r.second) (void)hipEventDestroy(r.second);
  ctx->readers.clear();
  ctx->readers.emplace_back(stream, nullptr);
  ctx->prepared.ordered_on = stream;
  ctx->prepared.ordered_valid = true;
  for (auto &t : ctx->prepared.tiles)
    if (t == 2) t = 1;
  return CUKING_OK;
}

// Marks plane tiles [begin, end) (units of 64 samples) as read by a kernel
// that has just been enqueued.
void mark_read(cuking_ctx *ctx, uint32_t begin, uint32_t end) {
  std::vector<uint8_t> &t = ctx->prepared.tiles;
  if (end > t.size()) end = (uint32_t)t.size();
  for (uint32_t k = begin; k < end; ++k) t[k] = 2;
}

bool same_block(const cuking_ctx::Prepared &p, const cuking_submatrix &sm,
                uint32_t words_per_sample, int variant, uint32_t tile, const uint64_t *bits) {
  return p.valid && p.sm.i_begin == sm.i_begin && p.sm.i_end == sm.i_end &&
         p.sm.j_begin == sm.j_begin && p.sm.j_end == sm.j_end &&
         p.words_per_sample == words_per_sample && p.variant == variant &&
         p.tile == tile && p.bits == bits;
}

// Makes the device buffer *buf (*bytes long) at least `need` bytes.  Replacing it waits
// for the whole device first: kernels of earlier calls (possibly on other streams) may
// still read the old one.
cuking_status grow(cuking_ctx *ctx, void **buf, size_t *bytes, size_t need) {
  if (need <= *bytes) return CUKING_OK;
  ++ctx->host_syncs;
  HIP_TRY(hipDeviceSynchronize());
  if (*buf) HIP_TRY(hipFree(*buf));
  *buf = nullptr;
  *bytes = 0;
  HIP_TRY(hipMalloc(buf, need));
  ++ctx->workspace_allocations;
  *bytes = need;
  return CUKING_OK;
}

// The workspace of the tiled kernel for `geo` / `tiles`: the planes, the band prefix
// and the sample sort's scratch.
cuking_status ensure_workspace(cuking_ctx *ctx, const PlaneGeometry &geo, const TiledVariant &v,
                               const TileSpace &tiles) {
  const size_t planes = plane_bytes(geo, v.layout);
  if (planes > ctx->planes_bytes) ctx->prepared.valid = false;
  cuking_status st = grow(ctx, reinterpret_cast<void **>(&ctx->planes), &ctx->planes_bytes, planes);
  if (st != CUKING_OK) return st;
  const size_t prefix = ((size_t)tiles.num_bands() + 1) * sizeof(uint64_t);
  if (prefix > ctx->band_prefix_bytes) ctx->prefix_for = TileSpace{0, 0, 0, 0};
  st = grow(ctx, reinterpret_cast<void **>(&ctx->band_prefix), &ctx->band_prefix_bytes, prefix);
  if (st != CUKING_OK || v.layout != kLayoutNibbleStats || ctx->filter_sort == 0) return st;
  return grow(ctx, &ctx->sort_temp, &ctx->sort_temp_bytes, sort_temp_bytes_for(geo.s_stride));
}

bool same_tile_space(const TileSpace &a, const TileSpace &b) {
  return a.tiles_r == b.tiles_r && a.tiles_c == b.tiles_c && a.band_rows == b.band_rows &&
         a.diag == b.diag;
}

// Uploads the band prefix of `tiles` (the caller has ordered `stream` behind
// the readers of the old one).
cuking_status upload_prefix(cuking_ctx *ctx, const TileSpace &tiles, hipStream_t stream) {
  const uint32_t nb = tiles.num_bands();
  std::vector<uint64_t> prefix((size_t)nb + 1, 0);
  for (uint32_t b = 0; b < nb; ++b) prefix[b + 1] = prefix[b] + tiles.band_tiles(b);
  // Small and pageable: wait until the host buffer may go away.
  HIP_TRY(hipMemcpyAsync(ctx->band_prefix, prefix.data(), prefix.size() * sizeof(uint64_t),
                         hipMemcpyHostToDevice, stream));
  ++ctx->host_syncs;
  HIP_TRY(hipStreamSynchronize(stream));
  ctx->prefix_for = tiles;
  return CUKING_OK;
}

// The nibble codes (+ het-only copy) of every converted tile of a kLayoutNibbleStats
// workspace whose last conversion left them out (lazy codes): for calls that run the
// four-product kernel directly.
cuking_status convert_codes_now(cuking_ctx *ctx, const PlaneGeometry &geo,
                                uint32_t words_per_sample, const uint64_t *d_bit_sets,
                                hipStream_t stream) {
  cuking_ctx::Prepared &pr = ctx->prepared;
  const uint32_t all = (uint32_t)pr.tiles.size();
  for (uint32_t t = 0; t < all;) {
    if (pr.tiles[t] == 0) {
      ++t;
      continue;
    }
    uint32_t e = t;
    while (e < all && pr.tiles[e] != 0) ++e;
    HIP_TRY(launch_prepare_nibbles(true, false, d_bit_sets, words_per_sample, geo, ctx->planes,
                                   plane_perm(ctx->planes, geo), t, e, nullptr, nullptr, stream));
    t = e;
  }
  HIP_TRY(hipMemsetAsync(plane_flags(ctx->planes, geo), 1, sizeof(uint32_t), stream));
  pr.codes = true;
  return CUKING_OK;
}

// What prepare() is asked for: plane samples [s_tile_begin, s_tile_end) (units of 64; the end
// is clamped to the block's) of block `sm` of a bitset, converted on `stream` for a call of
// `form` (king_launch_plan.h: an unsorted form's layout keeps stored order).  filter_call:
// the filter runs for the call (LaunchSwitches::filter_runs) at kin_threshold -- the site
// order may apply, and the four-product kernel's codes may stay unconverted.
struct PrepareRequest {
  const cuking_submatrix &sm;
  uint32_t words_per_sample;
  const uint64_t *d_bit_sets;
  hipStream_t stream;
  uint32_t s_tile_begin, s_tile_end;
  CallForm form;
  bool filter_call;
  float kin_threshold;
};
constexpr uint32_t kEveryPlaneTile = 0xFFFFFFFFu;

// Site order ("filter_site_order"), what the host knows in front of the conversion: whether
// this request's layout is to get its curve built (`wanted`), the scratch that takes, and the
// gather that would apply the order.
struct SiteOrderPlan {
  uint32_t num_stored;
  SiteOrderScratch layout;
  bool wanted;
  int gather;
};
// Whole-block conversions for a call the filter runs for.  Automatic: blocks of at least
// kSiteOrderMinTiles tiles whose bitset is long enough for check points get their curve
// built; whether the layout then takes the order is decided from the curve
// (decide_site_order).
SiteOrderPlan plan_site_order(const cuking_ctx *ctx, const PrepareRequest &rq, const TiledVariant &v,
                              const PlaneGeometry &geo, const TileSpace &tiles, bool whole) {
  SiteOrderPlan p = {};
  p.num_stored = geo.diag ? geo.num_rows : geo.num_rows + geo.num_cols;
  if (rq.filter_call && !kCallForms[rq.form].unsorted && v.layout == kLayoutNibbleStats &&
      ctx->filter_site_order != 0 && whole) {
    p.layout = site_order_scratch(p.num_stored, rq.words_per_sample);
    p.wanted = p.layout.bytes != 0 &&
               (ctx->filter_site_order >= 1 ||
                (total_tiles(tiles) >= ctx->filter_site_order_min_tiles &&
                 geo.k_words / 8 >= filter_check_min_steps()));
  }
  p.gather = site_gather_pick(ctx->filter_site_gather, rq.words_per_sample);
  return p;
}

// Site order, the decision for a layout that is about to be converted (*site_order: the
// layout takes the order): counts, weights, sort and the curve in this stream's scratch, and
// the host waits for the curve before it decides -- the order takes the layout when the
// option says 1, or when the curve forecasts the check at least kSiteOrderMinGain 64ths
// earlier than stored order has it and the launch-wide verdict does not send every tile away
// first.  The scratch (a second copy of the bitset among it) is allocated here, on first use
// and again for a larger block -- cuking_ctx_reserve does not know it.  A "no" has cost the
// counts, the sort and the wait, not the gather, and keeps rotated tiles.
cuking_status decide_site_order(cuking_ctx *ctx, const PrepareRequest &rq, const PlaneGeometry &geo,
                                const SiteOrderPlan &plan, bool *site_order) {
  cuking_ctx::Prepared &pr = ctx->prepared;
  *site_order = false;
  // (an automatic "no" is remembered for the block: conversion inside every pass of a
  //  cohort the order cannot help must not pay the counts, the sort and the wait each time)
  const bool trust_no = ctx->filter_site_order == -1 && pr.order_no_left != 0 &&
                        pr.order_thr == rq.kin_threshold;
  if (trust_no) --pr.order_no_left;
  if (plan.wanted && !trust_no) {
    cuking_ctx::StreamScratch *e = stream_entry(ctx, rq.stream);
    const cuking_status st = grow_on_stream(ctx, rq.stream, &e->site_order, plan.layout.bytes);
    if (st != CUKING_OK) return st;
    SiteCurve *d_curve = plane_site_curve(ctx->planes, geo);
    HIP_TRY(launch_site_order(rq.d_bit_sets, plan.num_stored, rq.words_per_sample, geo,
                              e->site_order.p, plan.layout, d_curve, rq.stream));
    SiteCurve curve;
    HIP_TRY(hipMemcpyAsync(&curve, d_curve, sizeof curve, hipMemcpyDeviceToHost, rq.stream));
    ++ctx->host_syncs;
    HIP_TRY(hipStreamSynchronize(rq.stream));
    const SiteOrderForecast f =
        site_order_forecast(curve, plan.num_stored, geo.k_words, rq.kin_threshold);
    ctx->order_forecast = f;
    ctx->order_sigma = curve.sigma;
    *site_order = ctx->filter_site_order >= 1 ||
                  (!f.verdict_first && f.order64 != 0 &&
                   (f.stored64 == 0 || f.order64 + kSiteOrderMinGain <= f.stored64));
    pr.order_thr = rq.kin_threshold;
    pr.order_no_left = *site_order ? 0u : kSiteOrderNoTrust;
  }
  pr.site_order = *site_order;
  return CUKING_OK;
}

// The filter variant's layout (kLayoutNibbleStats) for plane tiles [rq.s_tile_begin, t_end),
// step by step: statistics in stored order, the sample order (king_sort.hip), T2 -- and the
// four-product kernel's codes now, or by a gated launch behind the filter kernel if that
// turns out to need them (lazy codes: whole blocks only; the ranges of a staged pass are
// converted in full).
cuking_status convert_nibble_layout(cuking_ctx *ctx, const PrepareRequest &rq,
                                    const PlaneGeometry &geo, const SiteOrderPlan &plan,
                                    uint32_t t_end, bool whole) {
  cuking_ctx::Prepared &pr = ctx->prepared;
  hipStream_t stream = rq.stream;
  const bool codes = !rq.filter_call || !ctx->filter_lazy_codes || !whole;
  const uint32_t sb = rq.s_tile_begin * 64, se = t_end * 64;
  if (rq.s_tile_begin == 0)  // a conversion that starts at plane sample 0 starts the cohort's sums afresh
    HIP_TRY(hipMemsetAsync(const_cast<unsigned long long *>(plane_cohort_sums(ctx->planes, geo)),
                           0, 64, stream));
  // (whatever is converted now, the codes of the block as a whole are not "there" unless
  //  this conversion or convert_codes_now() below says so)
  HIP_TRY(hipMemsetAsync(plane_flags(ctx->planes, geo), 0, sizeof(uint32_t), stream));
  // Site order: the bitset with every sample's sites in that order in this stream's scratch
  // -- what the statistics and T2 are built from, so that both see the SAME order (one extra
  // write and read of the bitset, against a gather in each of the two kernels).  The codes
  // stay in stored order, like everything that recounts.
  bool site_order;
  cuking_status st = decide_site_order(ctx, rq, geo, plan, &site_order);
  if (st != CUKING_OK) return st;
  const uint64_t *layout_bits = rq.d_bit_sets;
  // The byte-wide gather of a diagonal block (plane sample = stored sample) counts the
  // statistics on the words it assembles: the separate kernel keeps the padding samples
  // behind the stored ones, which read nothing.
  const bool fused_stats = site_order && plan.gather > 0 && geo.diag != 0;
  if (site_order) {
    cuking_ctx::StreamScratch *e = stream_entry(ctx, stream);
    const SiteGatherStats fused = {stats_arrays(geo, ctx->planes), geo, se};
    HIP_TRY(launch_site_permute(rq.d_bit_sets, plan.num_stored, rq.words_per_sample,
                                e->site_order.p, plan.layout, plan.gather,
                                fused_stats ? &fused : nullptr, stream));
    layout_bits = reinterpret_cast<const uint64_t *>(static_cast<const uint8_t *>(e->site_order.p) +
                                                     plan.layout.permuted);
  }
  HIP_TRY(launch_sample_stats(layout_bits, rq.words_per_sample, geo, ctx->planes,
                              fused_stats ? plan.num_stored : sb, se, stream));
  HIP_TRY(launch_sample_order(geo, rq.words_per_sample, ctx->planes, sb, se,
                              !kCallForms[rq.form].unsorted &&
                                  (ctx->filter_sort == 2 || (ctx->filter_sort == 1 && whole)),
                              ctx->sort_temp, ctx->sort_temp_bytes, stream));
  HIP_TRY(launch_prepare_nibbles(codes && !site_order, true, layout_bits, rq.words_per_sample, geo,
                                 ctx->planes, plane_perm(ctx->planes, geo), rq.s_tile_begin, t_end,
                                 nullptr, nullptr, stream));
  if (codes && site_order)
    HIP_TRY(launch_prepare_nibbles(true, false, rq.d_bit_sets, rq.words_per_sample, geo,
                                   ctx->planes, plane_perm(ctx->planes, geo), rq.s_tile_begin,
                                   t_end, nullptr, nullptr, stream));
  if (!codes) {
    pr.codes = false;
  } else if (!pr.codes) {
    // earlier tiles of this block were converted without codes: complete them
    return convert_codes_now(ctx, geo, rq.words_per_sample, rq.d_bit_sets, stream);
  } else {
    HIP_TRY(hipMemsetAsync(plane_flags(ctx->planes, geo), 1, sizeof(uint32_t), stream));
  }
  return CUKING_OK;
}

// Builds planes + band prefix for `rq.sm` in the context workspace: the workspace, the
// "same block?" decision, the ordering against readers, the prefix, then the conversion.
cuking_status prepare(cuking_ctx *ctx, const PrepareRequest &rq, PlaneGeometry *geo_out,
                      TileSpace *tiles_out) {
  const cuking_submatrix &sm = rq.sm;
  const uint32_t words_per_sample = rq.words_per_sample;
  hipStream_t stream = rq.stream;
  const int variant = effective_variant(ctx, words_per_sample);
  const TiledVariant v = plan_variant(ctx, words_per_sample);
  const PlaneGeometry geo = make_geometry(sm, words_per_sample, v);
  const TileSpace tiles = make_tiles(geo, v, ctx->band_rows);
  *geo_out = geo;
  *tiles_out = tiles;

  cuking_status st = ensure_workspace(ctx, geo, v, tiles);
  if (st != CUKING_OK) return st;
  // Book-keeping of what the workspace holds, and ordering against kernels on
  // other streams that still read what is about to be overwritten -- the planes
  // AND the band prefix below, so this comes before either is touched.
  const uint32_t all_tiles = (geo.s_stride + 63) / 64;
  const uint32_t s_tile_begin = rq.s_tile_begin;
  const uint32_t t_end = rq.s_tile_end < all_tiles ? rq.s_tile_end : all_tiles;
  const bool whole = s_tile_begin == 0 && t_end == all_tiles;
  cuking_ctx::Prepared &pr = ctx->prepared;
  const bool new_prefix = !same_tile_space(ctx->prefix_for, tiles);
  const bool dense_order = kCallForms[rq.form].unsorted;
  const SiteOrderPlan order = plan_site_order(ctx, rq, v, geo, tiles, whole);
  if (order.wanted && order.gather < 0)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "filter_site_gather %d: %u words per sample do not fit the gather's LDS",
                       ctx->filter_site_gather, words_per_sample);
  // (a layout converted for an unsorted form is unsorted: a call of the other kind treats it
  //  as another block's, and the other way round ... and a layout converted under another
  //  answer to "is the curve wanted" is another block's as well.  A layout that is reused
  //  keeps the decision of the call that converted it, whatever threshold this one has: its
  //  share comes from the curve and this call's threshold.)
  const bool same = same_block(pr, sm, words_per_sample, variant, v.tile, rq.d_bit_sets) &&
                    pr.dense_order == dense_order && pr.order_wanted == order.wanted &&
                    // (the share of an ordered layout comes from its curve at the call's
                    //  threshold and may be "no check at all" at another one, where stored
                    //  order would have had one: such a call decides and converts afresh)
                    !(pr.site_order && pr.order_thr != rq.kin_threshold);
  if (ctx->reuse_prepared && same && !new_prefix) {
    // The host has promised that the bitset behind this pointer is unchanged
    // since it was converted (cuking_invalidate otherwise): nothing to do when
    // every tile asked for is there.
    bool all_there = true;
    for (uint32_t t = s_tile_begin; t < t_end && all_there; ++t) all_there = pr.tiles[t] != 0;
    if (all_there) {
      ++ctx->conversions_skipped;
      if (v.layout == kLayoutNibbleStats && !rq.filter_call && !pr.codes)
        return convert_codes_now(ctx, geo, words_per_sample, rq.d_bit_sets, stream);
      return CUKING_OK;
    }
  }
  // Needs ordering: a conversion for another block while anything may still
  // read the old one; a repeated conversion of tiles that kernels enqueued
  // since have read (2); or of tiles whose readers were last ordered behind a
  // different stream (1).  Fresh tiles of the same block have no readers.
  const bool other_stream = pr.ordered_valid && pr.ordered_on != stream;
  bool must_wait = new_prefix && !ctx->readers.empty();
  if (!same) {
    must_wait = must_wait || !ctx->readers.empty();
    pr.valid = true;
    pr.sm = sm;
    pr.words_per_sample = words_per_sample;
    pr.variant = variant;
    pr.tile = v.tile;
    pr.bits = rq.d_bit_sets;
    pr.tiles.assign(all_tiles, 0);
    pr.codes = true;
    pr.dense_order = dense_order;
    pr.order_wanted = order.wanted;
    pr.site_order = false;
    pr.order_no_left = 0;
  }
  for (uint32_t t = s_tile_begin; t < t_end; ++t)
    must_wait = must_wait || pr.tiles[t] == 2 || (pr.tiles[t] == 1 && other_stream);
  if (must_wait) {
    st = wait_for_readers(ctx, stream);
    if (st != CUKING_OK) return st;
  }
  for (uint32_t t = s_tile_begin; t < t_end; ++t) pr.tiles[t] = 1;
  if (new_prefix) {
    st = upload_prefix(ctx, tiles, stream);
    if (st != CUKING_OK) return st;
  }

  if (plane_bytes(geo, v.layout) == 0) return CUKING_OK;
  EventPair *ev = nullptr;
  if (ctx->timing) HIP_TRY(ctx->prepare_timer.begin(stream, &ev));
  if (v.layout == kLayoutNibbleStats) {
    st = convert_nibble_layout(ctx, rq, geo, order, t_end, whole);
    if (st != CUKING_OK) return st;
  } else {
    HIP_TRY(launch_prepare_planes(v.layout, rq.d_bit_sets, words_per_sample, geo, ctx->planes,
                                  s_tile_begin, rq.s_tile_end, stream));
  }
  if (ev) HIP_TRY(hipEventRecord(ev->stop, stream));
  return CUKING_OK;
}

// The block a pair call works on, as every entry point receives it.
struct BlockArgs {
  cuking_ctx *ctx;
  const cuking_submatrix *sm;
  uint32_t words_per_sample;
  const uint64_t *d_bit_sets;
  void *stream;
};
// Every tile of the block (the only form the stream kernel serves), or tiles [begin, end) of
// its enumeration.
struct TileRange {
  bool whole;
  uint64_t begin, end;
};
constexpr TileRange kEveryTile = {true, 0, 0};

// The tiled kernels for a call of out.form: what the form's rules (king_launch_plan.h
// kCallForms) say about the k loop, the layout and the filter, then conversion and launch.
cuking_status run_tiled(const BlockArgs &b, TileRange r, const Outputs &out) {
  cuking_ctx *ctx = b.ctx;
  const cuking_submatrix &sm = *b.sm;
  hipStream_t stream = (hipStream_t)b.stream;
  const CallFormRules &rules = kCallForms[out.form];
  const bool mfma = is_mfma_variant(effective_variant(ctx, b.words_per_sample));
  // (the entry points of these forms have refused every other context)
  if (!mfma && !rules.valu_serves)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "%s: no matrix-core kernel", rules.name);
  // (a form that keeps every pair on the lean k loop does so on the matrix cores: the VALU
  //  kernels store a matrix from their full form)
  const bool full = rules.k_loop == kLoopEither
                        ? use_full_counts(ctx, out.kin_threshold, b.words_per_sample)
                        : rules.k_loop == kLoopFull || !mfma;
  const LaunchSwitches sw =
      launch_switches(ctx, b.words_per_sample, out.form, full, out.kin_threshold);
  PlaneGeometry geo;
  TileSpace tiles;
  cuking_status st = prepare(ctx,
                             {sm, b.words_per_sample, b.d_bit_sets, stream, 0, kEveryPlaneTile,
                              out.form, sw.filter_runs, out.kin_threshold},
                             &geo, &tiles);
  if (st != CUKING_OK) return st;
  const uint64_t n_tiles = total_tiles(tiles);
  if (r.whole) r = {true, 0, n_tiles};
  if (r.begin > r.end || r.end > n_tiles)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                "tile range [%llu, %llu) outside [0, %llu)",
                (unsigned long long)r.begin, (unsigned long long)r.end,
                (unsigned long long)n_tiles);
  if (r.begin == r.end) return CUKING_OK;

  TiledArgs a;
  st = launch_args(ctx, stream, sm, b.words_per_sample, b.d_bit_sets, geo, tiles, n_tiles, out, &a);
  if (st != CUKING_OK) return st;
  a.tile_begin = r.begin;

  EventPair *ev = nullptr;
  if (ctx->timing) HIP_TRY(ctx->king_timer.begin(stream, &ev));
  HIP_TRY(launch_planned(ctx, b.words_per_sample, full, a, sw, r.end - r.begin, stream));
  note_reader(ctx, stream);
  mark_read(ctx, 0, 0xFFFFFFFFu);
  if (a.kin_diag != 0) HIP_TRY(launch_kin_mirror(out.kin, out.kin_ld, geo.num_rows, stream));
  if (ev) HIP_TRY(hipEventRecord(ev->stop, stream));
  return CUKING_OK;
}

// The stream kernel, for the whole block and the forms the VALU kernels serve.
cuking_status run_stream(const BlockArgs &b, const Outputs &out) {
  cuking_ctx *ctx = b.ctx;
  hipStream_t stream = (hipStream_t)b.stream;
  EventPair *ev = nullptr;
  if (ctx->timing) HIP_TRY(ctx->king_timer.begin(stream, &ev));
  const uint32_t kin_diag =
      (out.kin != nullptr && (out.kin_flags & CUKING_KIN_SYMMETRIC)) ? 1u : 0u;
  HIP_TRY(launch_stream(*b.sm, b.words_per_sample, b.d_bit_sets, out.kin_threshold,
                        out.max_results, out.results, out.result_index, out.result_overflow,
                        out.counts, out.kin, out.kin_ld, kin_diag, stream));
  if (kin_diag != 0) HIP_TRY(launch_kin_mirror(out.kin, out.kin_ld, sm_num_rows(*b.sm), stream));
  if (ev) HIP_TRY(hipEventRecord(ev->stop, stream));
  return CUKING_OK;
}

// Where a call binds its context's device, among the steps every call takes.  The calls
// differ in it (and so in what an invalid call with a null context, or one that meets a
// device error, reports first); the difference is kept as it was, not decided here.
enum class BindAt { kFirst, kBehindCheck, kBehindEmptyBlock };

// What the pair calls X and X_tiles share, for every X: the call's own part `check` (its
// argument checks, then its Outputs), the empty block's rule, the kernel.
template <class Check>
cuking_status run_pair_call(const BlockArgs &b, const TileRange &r, BindAt bind_at, Check check) {
  if (bind_at == BindAt::kFirst) BIND_OR_RETURN(b.ctx);
  Outputs out = {};
  const cuking_status st = check(&out);
  if (st != CUKING_OK) return st;
  if (bind_at == BindAt::kBehindCheck) BIND_OR_RETURN(b.ctx);
  if (sm_num_rows(*b.sm) == 0 || sm_num_cols(*b.sm) == 0) {
    // (the checks of the matrix-core-only forms have refused such a range already, in the
    //  words of every range outside the block's)
    if (!r.whole && (r.begin != 0 || r.end != 0))
      return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "empty block has no tiles");
    return CUKING_OK;
  }
  if (bind_at == BindAt::kBehindEmptyBlock) BIND_OR_RETURN(b.ctx);
  if (r.whole && b.ctx->kernel == CUKING_KERNEL_STREAM) return run_stream(b, out);
  return run_tiled(b, r, out);
}

// ---- options ---------------------------------------------------------------

// What setting an option does besides storing the value.
enum : uint8_t {
  kInvalidatesLayout = 1,  // the prepared layout was built under the old value
  kResizesSlabs = 2,       // split slabs are sized by it: a change frees them (waits for the device)
};

struct Option {
  const char *key;
  int64_t lo, hi;          // accepted values, inclusive ...
  const char *error;       // ... and the message for any other (%u: error_arg)
  uint32_t error_arg;
  uint8_t effects;
  int64_t (*get)(const cuking_ctx *);
  void (*set)(cuking_ctx *, int64_t);
  int64_t hole = INT64_MIN;  // a value inside the bounds that is refused as well
  bool (*valid)(int64_t) = nullptr;  // what else a value inside the bounds must satisfy
};

// Reads and stores a field of the context.
#define CTX_FIELD(f)                                                     \
  [](const cuking_ctx *c) -> int64_t { return (int64_t)c->f; },          \
  [](cuking_ctx *c, int64_t v) { c->f = (decltype(c->f))v; }

// The settable options (include/cuking_amd.h documents them in this order).  None of them
// changes any record.
const Option kOptions[] = {
    {"variant", 0, kNumTiledVariants - 1, "variant outside [0, %u)", kNumTiledVariants, 0,
     CTX_FIELD(variant)},
    {"band_rows", 0, 64, "band_rows outside [0, 64]", 0, 0, CTX_FIELD(band_rows)},
    {"counts_mode", -1, 1, "counts_mode outside [-1, 1]", 0, 0, CTX_FIELD(counts_mode)},
    {"split_wgs", 0, 4096, "split_wgs outside [0, 4096]", 0, kResizesSlabs, CTX_FIELD(split_wgs)},
    {"xcd_swizzle", 0, 2, "xcd_swizzle outside [0, 2]", 0, 0, CTX_FIELD(xcd_swizzle)},
    {"dyn_tail_tiles", 0, 0x7FFFFFFF, "dyn_tail_tiles outside [0, 2^31)", 0, 0,
     CTX_FIELD(dyn_tail_tiles)},
    {"reuse_prepared", 0, 1, "reuse_prepared outside [0, 1]", 0, 0, CTX_FIELD(reuse_prepared)},
    {"filter_sort", 0, 2, "filter_sort outside [0, 2]", 0, kInvalidatesLayout,
     CTX_FIELD(filter_sort)},
    {"filter_lazy_codes", 0, 1, "filter_lazy_codes outside [0, 1]", 0, kInvalidatesLayout,
     CTX_FIELD(filter_lazy_codes)},
    {"filter_site_order", -1, 2, "filter_site_order outside [-1, 2]", 0, kInvalidatesLayout,
     CTX_FIELD(filter_site_order)},
    {"filter_site_order_min_tiles", 0, 1 << 30, "filter_site_order_min_tiles outside [0, 2^30]",
     0, kInvalidatesLayout, CTX_FIELD(filter_site_order_min_tiles)},
    {"filter_site_gather", -1, 4, "filter_site_gather outside {-1, 0, 2, 4}", 0,
     kInvalidatesLayout, CTX_FIELD(filter_site_gather), /*hole=*/INT64_MIN,
     [](int64_t v) { return v == -1 || (v & 1) == 0; }},
    {"filter_check0", 0, 2, "filter_check0 outside [0, 2]", 0, 0, CTX_FIELD(filter_check0)},
    {"filter_check1", 0, 1 + kNumCheckShares, "filter_check1 outside {0, 1, 3 .. %u}",
     1 + kNumCheckShares, 0, CTX_FIELD(filter_check1), /*hole=*/2},
    {"filter_check_emit", 0, 255, "filter_check_emit outside [0, 255]", 0, 0,
     CTX_FIELD(filter_check_emit)},
    {"filter_rotate", 0, 2 + kNumPhases, "filter_rotate outside [0, %u]", 2 + kNumPhases, 0,
     CTX_FIELD(filter_rotate)},
    {"filter_rotate_min_steps", 1, 1 << 20, "filter_rotate_min_steps outside [1, 2^20]", 0, 0,
     CTX_FIELD(filter_rotate_min_steps)},
    {"filter_rotate_min_tiles", 0, 1 << 30, "filter_rotate_min_tiles outside [0, 2^30]", 0, 0,
     CTX_FIELD(filter_rotate_min_tiles)},
    // test hooks: force the paths of the filter variant that ordinary cohorts do not take
    {"filter_quadrant_cap", 0, 16384, "filter_quadrant_cap outside [0, 16384]", 0, 0,
     CTX_FIELD(filter_quadrant_cap)},
    {"filter_cand_cap", 0, kFilterCandCap, "filter_cand_cap outside [0, %u]", kFilterCandCap, 0,
     CTX_FIELD(filter_cand_cap)},
    {"filter_split_min_steps", 1, 4096, "filter_split_min_steps outside [1, 4096]", 0, 0,
     CTX_FIELD(filter_split_min_steps)},
    // test hooks of the whole process, not of the context
    {"max_launch_blocks", 0, INT64_MAX, "negative block cap", 0, 0,
     [](const cuking_ctx *) -> int64_t { return (int64_t)max_blocks_override(); },
     [](cuking_ctx *, int64_t v) { set_max_blocks_per_launch((uint64_t)v); }},
    {"filter_check_min_steps", 4, 1 << 20, "filter_check_min_steps outside [4, 2^20]", 0,
     kInvalidatesLayout,  // (the prefix counts of the workspace belong to the old value)
     [](const cuking_ctx *) -> int64_t { return filter_check_min_steps(); },
     [](cuking_ctx *, int64_t v) { set_filter_check_min_steps((uint32_t)v); }},
};
#undef CTX_FIELD

const Option *find_option(const char *key) {
  for (const Option &o : kOptions)
    if (strcmp(o.key, key) == 0) return &o;
  return nullptr;
}

// The read-only keys of cuking_ctx_get_option.
cuking_status read_diagnostic(const cuking_ctx *ctx, const char *key, int64_t *value) {
  const std::pair<const char *, uint64_t> counters[] = {
      {"workspace_allocations", ctx->workspace_allocations},
      {"host_syncs", ctx->host_syncs},
      {"conversions_skipped", ctx->conversions_skipped},
      // (site order: what the last conversion that built a curve read from it -- the share
      //  of an unrotated tile's check in 64ths by the curve and by stored order's rule, 0 =
      //  none; the counts' sigma in millionths; whether the prepared layout took the order)
      {"site_order_share", ctx->order_forecast.order64},
      {"site_order_stored_share", ctx->order_forecast.stored64},
      {"site_order_sigma_e6", (uint64_t)llroundf(ctx->order_sigma * 1e6f)},
      {"site_order_on", ctx->prepared.valid && ctx->prepared.site_order ? 1u : 0u}};
  for (const auto &c : counters)
    if (strcmp(c.first, key) == 0) {
      *value = (int64_t)c.second;
      return CUKING_OK;
    }
  // Diagnostics of the filter variant, summed over the context's streams (they WAIT for the
  // device): pairs the bound let through, quadrants handed to the exact kernel, tiles that
  // left at the rigorous check point and tiles that started at another phase, since the
  // context was created ...
  const char *const totals[kNumTotals] = {"filter_candidates", "filter_dense_quadrants",
                                          "filter_early_exits", "filter_rotated_tiles"};
  static_assert(kTotalCand == 0 && kTotalDense == 1 && kTotalEarly == 2 && kTotalRotated == 3,
                "totals[] in the order of the running totals");
  uint32_t word = 0;
  while (word < kNumTotals && strcmp(totals[word], key) != 0) ++word;
  // ... and the 100 MHz counter's ticks per k-step x 16 as the tiles of the last launch chunk
  // measured them (rotated tiles, king_filter.hip), averaged over the XCDs that said so and
  // the context's streams; 0 = nobody did.
  const bool ticks = strcmp(key, "filter_step_ticks16") == 0;
  if (word == kNumTotals && !ticks)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "unknown option %s", key);
  if (hipSetDevice(ctx->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
    return cuking_fail(CUKING_ERR_DEVICE, "device wait failed");
  unsigned long long sum = 0;
  uint64_t count = 0;
  for (const auto &e : ctx->scratch) {
    if (e.filter == nullptr) continue;
    if (ticks) {
      uint32_t w[8];
      if (hipMemcpy(w, e.filter + kCtrlStepTicks * 4, sizeof w, hipMemcpyDeviceToHost) != hipSuccess)
        return cuking_fail(CUKING_ERR_DEVICE, "reading the filter counters failed");
      for (uint32_t v : w)
        if (v != 0) {
          sum += v;
          ++count;
        }
    } else {
      unsigned long long v = 0;
      if (hipMemcpy(&v, e.filter + filter_scratch_layout(e.filter_tiles).totals + word * 8, 8,
                    hipMemcpyDeviceToHost) != hipSuccess)
        return cuking_fail(CUKING_ERR_DEVICE, "reading the filter counters failed");
      sum += v;
    }
  }
  if (ticks) *value = count != 0 ? (int64_t)(sum / count) : 0;
  else *value = (int64_t)(sum + ctx->filter_totals_retired[word]);
  return CUKING_OK;
}

}  // namespace

extern "C" {

// ---- context and memory ---------------------------------------------------

int cuking_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

cuking_status cuking_ctx_create(int device, cuking_ctx **out) {
  if (out == nullptr) return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null out pointer");
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n == 0)
    return cuking_fail(CUKING_ERR_DEVICE,
                "no HIP device available (%s); this library has no CPU path",
                e == hipSuccess ? "0 devices" : hipGetErrorString(e));
  if (device < 0 || device >= n)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "device %d outside [0, %d)", device, n);
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return cuking_fail(CUKING_ERR_DEVICE,
                "device %d is %s; this library only carries gfx950 code",
                device, prop.gcnArchName);
  HIP_TRY(hipSetDevice(device));
  cuking_ctx *ctx = new cuking_ctx();
  ctx->device = device;
  ctx->variant = default_variant();
  ctx->split_wgs = (uint32_t)prop.multiProcessorCount;
  ctx->num_cus = (uint32_t)prop.multiProcessorCount;
  *out = ctx;
  return CUKING_OK;
}

void cuking_ctx_destroy(cuking_ctx *ctx) {
  if (ctx == nullptr) return;
  (void)hipSetDevice(ctx->device);
  if (ctx->planes) (void)hipFree(ctx->planes);
  if (ctx->band_prefix) (void)hipFree(ctx->band_prefix);
  if (ctx->sort_temp) (void)hipFree(ctx->sort_temp);
  if (ctx->synth_tables) (void)hipFree(ctx->synth_tables);
  if (ctx->synth_done) (void)hipEventDestroy(ctx->synth_done);
  // (nobody reads the filter's totals any more: they are not copied back)
  for (auto &e : ctx->scratch) free_stream_scratch(ctx, e, false);
  for (auto &r : ctx->readers)
    if (r.second) (void)hipEventDestroy(r.second);
  ctx->king_timer.destroy();
  ctx->prepare_timer.destroy();
  delete ctx;
}

cuking_status cuking_ctx_set_kernel(cuking_ctx *ctx, cuking_kernel kernel) {
  if (ctx == nullptr) return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null context");
  if (kernel != CUKING_KERNEL_TILED && kernel != CUKING_KERNEL_STREAM)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "unknown kernel %d", (int)kernel);
  ctx->kernel = kernel;
  return CUKING_OK;
}

cuking_status cuking_ctx_set_option(cuking_ctx *ctx, const char *key,
                                    int64_t value) {
  if (ctx == nullptr || key == nullptr)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null argument");
  const Option *o = find_option(key);
  if (o == nullptr) return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "unknown option %s", key);
  if (value < o->lo || value > o->hi || value == o->hole || (o->valid && !o->valid(value)))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, o->error, o->error_arg);
  if ((o->effects & kResizesSlabs) && value != o->get(ctx)) {
    HIP_TRY(hipDeviceSynchronize());
    for (auto &e : ctx->scratch) free_split_slab(e);
  }
  o->set(ctx, value);
  if (o->effects & kInvalidatesLayout) ctx->prepared.valid = false;
  return CUKING_OK;
}

cuking_status cuking_device_alloc(cuking_ctx *ctx, size_t bytes, void **d_ptr) {
  BIND_OR_RETURN(ctx);
  if (d_ptr == nullptr) return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null out pointer");
  *d_ptr = nullptr;
  if (bytes == 0) return CUKING_OK;
  HIP_TRY(hipMalloc(d_ptr, bytes));
  return CUKING_OK;
}

cuking_status cuking_device_free(cuking_ctx *ctx, void *d_ptr) {
  BIND_OR_RETURN(ctx);
  if (d_ptr) HIP_TRY(hipFree(d_ptr));
  return CUKING_OK;
}

cuking_status cuking_memset_async(cuking_ctx *ctx, void *d_ptr, int byte_value,
                                  size_t bytes, void *stream) {
  BIND_OR_RETURN(ctx);
  if (bytes) HIP_TRY(hipMemsetAsync(d_ptr, byte_value, bytes, (hipStream_t)stream));
  return CUKING_OK;
}

cuking_status cuking_copy_to_device(cuking_ctx *ctx, void *d_dst,
                                    const void *src, size_t bytes,
                                    void *stream) {
  BIND_OR_RETURN(ctx);
  if (bytes)
    HIP_TRY(hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice,
                           (hipStream_t)stream));
  return CUKING_OK;
}

cuking_status cuking_copy_to_host(cuking_ctx *ctx, void *dst, const void *d_src,
                                  size_t bytes, void *stream) {
  BIND_OR_RETURN(ctx);
  if (bytes)
    HIP_TRY(hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost,
                           (hipStream_t)stream));
  return CUKING_OK;
}

cuking_status cuking_stream_synchronize(cuking_ctx *ctx, void *stream) {
  BIND_OR_RETURN(ctx);
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  return CUKING_OK;
}

cuking_status cuking_stream_create(cuking_ctx *ctx, void **stream) {
  BIND_OR_RETURN(ctx);
  if (stream == nullptr) return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null out pointer");
  hipStream_t s = nullptr;
  HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  *stream = s;
  return CUKING_OK;
}

cuking_status cuking_stream_destroy(cuking_ctx *ctx, void *stream) {
  BIND_OR_RETURN(ctx);
  if (stream) {
    // hipStreamDestroy lets the stream's work finish; nothing may name it later.
    auto &rs = ctx->readers;
    for (size_t k = 0; k < rs.size(); ++k)
      if (rs[k].first == (hipStream_t)stream) {
        HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
        if (rs[k].second) (void)hipEventDestroy(rs[k].second);
        rs.erase(rs.begin() + k);
        break;
      }
    HIP_TRY(hipStreamDestroy((hipStream_t)stream));
  }
  return CUKING_OK;
}

cuking_status cuking_host_alloc(cuking_ctx *ctx, size_t bytes, void **ptr) {
  BIND_OR_RETURN(ctx);
  if (ptr == nullptr) return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null out pointer");
  *ptr = nullptr;
  if (bytes == 0) return CUKING_OK;
  HIP_TRY(hipHostMalloc(ptr, bytes, hipHostMallocDefault));
  return CUKING_OK;
}

cuking_status cuking_host_free(cuking_ctx *ctx, void *ptr) {
  BIND_OR_RETURN(ctx);
  if (ptr) HIP_TRY(hipHostFree(ptr));
  return CUKING_OK;
}

// ---- hot path -------------------------------------------------------------

cuking_status cuking_pack_device(cuking_ctx *ctx, const cuking_submatrix *sm,
                                 uint32_t words_per_sample, uint64_t *d_bit_set,
                                 const int64_t *d_row_idx,
                                 const int64_t *d_col_idx,
                                 const int32_t *d_n_alt_alleles,
                                 size_t num_triples, uint32_t *d_status,
                                 void *stream) {
  BIND_OR_RETURN(ctx);
  cuking_status st = cuking_check_block(sm, words_per_sample);
  if (st != CUKING_OK) return st;
  if (num_triples &&
      (!d_bit_set || !d_row_idx || !d_col_idx || !d_n_alt_alleles || !d_status))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null device pointer");
  HIP_TRY(launch_pack(*sm, words_per_sample, d_bit_set, d_row_idx, d_col_idx,
                      d_n_alt_alleles, num_triples, d_status,
                      (hipStream_t)stream));
  return CUKING_OK;
}

cuking_status cuking_pack_device_compact(cuking_ctx *ctx, const cuking_submatrix *sm,
                                         uint32_t words_per_sample, uint64_t *d_bit_set,
                                         const uint32_t *d_site,
                                         const uint32_t *d_sample_alt, size_t num_triples,
                                         uint32_t *d_status, void *stream) {
  BIND_OR_RETURN(ctx);
  cuking_status st = cuking_check_block(sm, words_per_sample);
  if (st != CUKING_OK) return st;
  if (num_triples && (!d_bit_set || !d_site || !d_sample_alt || !d_status))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null device pointer");
  HIP_TRY(launch_pack_compact(words_per_sample, sm_num_samples(*sm), d_bit_set, d_site,
                              d_sample_alt, num_triples, d_status, (hipStream_t)stream));
  return CUKING_OK;
}

cuking_status cuking_pack_bed_device(cuking_ctx *ctx, const cuking_submatrix *sm,
                                     uint32_t words_per_sample, uint64_t *d_bit_set,
                                     const uint8_t *d_bed_rows, uint64_t row_bytes,
                                     uint32_t site_begin, uint32_t site_end, uint32_t num_sites,
                                     void *stream) {
  // (the arguments first: a refused call touches no device)
  if (ctx == nullptr) return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null context");
  cuking_status st = cuking_check_bed_args(sm, words_per_sample, d_bit_set, d_bed_rows, row_bytes,
                                           site_begin, site_end, num_sites);
  if (st != CUKING_OK) return st;
  if (site_begin == site_end || sm_num_samples(*sm) == 0) return CUKING_OK;
  BIND_OR_RETURN(ctx);
  HIP_TRY(launch_pack_bed(*sm, words_per_sample, d_bit_set, d_bed_rows, row_bytes, site_begin,
                          site_end, (hipStream_t)stream));
  return CUKING_OK;
}

cuking_status cuking_event_create(cuking_ctx *ctx, void **event) {
  BIND_OR_RETURN(ctx);
  if (event == nullptr) return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null out pointer");
  hipEvent_t e = nullptr;
  HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  *event = e;
  return CUKING_OK;
}

cuking_status cuking_event_record(cuking_ctx *ctx, void *event, void *stream) {
  BIND_OR_RETURN(ctx);
  HIP_TRY(hipEventRecord((hipEvent_t)event, (hipStream_t)stream));
  return CUKING_OK;
}

cuking_status cuking_event_synchronize(cuking_ctx *ctx, void *event) {
  BIND_OR_RETURN(ctx);
  HIP_TRY(hipEventSynchronize((hipEvent_t)event));
  return CUKING_OK;
}

cuking_status cuking_event_destroy(cuking_ctx *ctx, void *event) {
  BIND_OR_RETURN(ctx);
  if (event) HIP_TRY(hipEventDestroy((hipEvent_t)event));
  return CUKING_OK;
}

uint32_t cuking_tile_samples(const cuking_ctx *ctx) {
  return tiled_variant(ctx ? ctx->variant : default_variant()).tile;
}

uint64_t cuking_num_tiles(const cuking_ctx *ctx, const cuking_submatrix *sm) {
  if (sm == nullptr) return 0;
  const TiledVariant &v = tiled_variant(ctx ? ctx->variant : default_variant());
  const PlaneGeometry g = make_geometry(*sm, 2, v);
  if (g.num_rows == 0 || g.num_cols == 0) return 0;
  return total_tiles(make_tiles(g, v, ctx ? ctx->band_rows : 0));
}

cuking_status cuking_tile_bounds(const cuking_ctx *ctx,
                                 const cuking_submatrix *sm, uint64_t tile,
                                 uint32_t *row_begin, uint32_t *row_end,
                                 uint32_t *col_begin, uint32_t *col_end) {
  cuking_status st = cuking_check_block(sm, 2);
  if (st != CUKING_OK) return st;
  const TiledVariant &v = tiled_variant(ctx ? ctx->variant : default_variant());
  const PlaneGeometry g = make_geometry(*sm, 2, v);
  const TileSpace ts = make_tiles(g, v, ctx ? ctx->band_rows : 0);
  if (g.num_rows == 0 || g.num_cols == 0 || tile >= total_tiles(ts))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "tile index out of range");
  uint32_t b = 0;
  uint64_t first = 0;
  while (first + ts.band_tiles(b) <= tile) first += ts.band_tiles(b++);
  uint32_t tr, tc;
  ts.decode(b, tile - first, &tr, &tc);
  auto clampr = [&](uint64_t x) { return (uint32_t)std::min<uint64_t>(x, g.num_rows); };
  auto clampc = [&](uint64_t x) { return (uint32_t)std::min<uint64_t>(x, g.num_cols); };
  if (row_begin) *row_begin = sm->i_begin + clampr((uint64_t)tr * v.tile);
  if (row_end) *row_end = sm->i_begin + clampr((uint64_t)(tr + 1) * v.tile);
  if (col_begin) *col_begin = sm->j_begin + clampc((uint64_t)tc * v.tile);
  if (col_end) *col_end = sm->j_begin + clampc((uint64_t)(tc + 1) * v.tile);
  return CUKING_OK;
}

cuking_status cuking_ctx_get_option(const cuking_ctx *ctx, const char *key,
                                    int64_t *value) {
  if (ctx == nullptr || key == nullptr || value == nullptr)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null argument");
  if (const Option *o = find_option(key)) {
    *value = o->get(ctx);
    return CUKING_OK;
  }
  return read_diagnostic(ctx, key, value);
}

int cuking_num_variants(void) { return kNumTiledVariants; }
const char *cuking_variant_name(int variant) {
  if (variant < 0 || variant >= kNumTiledVariants) return "";
  return tiled_variant(variant).name;
}

static cuking_status check_compute_args(const cuking_submatrix *sm,
                                        uint32_t words_per_sample,
                                        const uint64_t *d_bit_sets) {
  cuking_status st = cuking_check_block(sm, words_per_sample);
  if (st != CUKING_OK) return st;
  if (sm_num_samples(*sm) != 0 && d_bit_sets == nullptr)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null bitset pointer");
  return CUKING_OK;
}

// cuking_compute_king and cuking_compute_king_tiles.  (Binds first: a null context is
// reported in front of any bad argument.)
static cuking_status king_call(const BlockArgs &b, const TileRange &r, float kin_threshold,
                               uint32_t max_results, cuking_result *d_results,
                               uint32_t *d_result_index, uint32_t *d_result_overflow) {
  return run_pair_call(b, r, BindAt::kFirst, [&](Outputs *out) {
    const cuking_status st = check_compute_args(b.sm, b.words_per_sample, b.d_bit_sets);
    if (st != CUKING_OK) return st;
    if (!d_result_index || !d_result_overflow || (max_results && !d_results))
      return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null result pointer");
    *out = record_outputs(kFormRecords, kin_threshold, max_results, d_results, d_result_index,
                          d_result_overflow);
    return CUKING_OK;
  });
}

cuking_status cuking_compute_king(cuking_ctx *ctx, const cuking_submatrix *sm,
                                  uint32_t words_per_sample,
                                  const uint64_t *d_bit_sets,
                                  float kin_threshold, uint32_t max_results,
                                  cuking_result *d_results,
                                  uint32_t *d_result_index,
                                  uint32_t *d_result_overflow, void *stream) {
  return king_call({ctx, sm, words_per_sample, d_bit_sets, stream}, kEveryTile, kin_threshold,
                   max_results, d_results, d_result_index, d_result_overflow);
}

cuking_status cuking_compute_king_tiles(
    cuking_ctx *ctx, const cuking_submatrix *sm, uint32_t words_per_sample,
    const uint64_t *d_bit_sets, uint64_t tile_begin, uint64_t tile_end,
    float kin_threshold, uint32_t max_results, cuking_result *d_results,
    uint32_t *d_result_index, uint32_t *d_result_overflow, void *stream) {
  return king_call({ctx, sm, words_per_sample, d_bit_sets, stream}, {false, tile_begin, tile_end},
                   kin_threshold, max_results, d_results, d_result_index, d_result_overflow);
}

// Offsets of a sample range inside a diagonal block, in tiles.
static cuking_status tile_span(const cuking_submatrix &sm, uint32_t tile,
                               uint32_t begin, uint32_t end, const char *what,
                               uint32_t *t0, uint32_t *t1) {
  if (begin < sm.i_begin || end > sm.i_end || begin > end)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "%s range [%u, %u) outside the block",
                what, begin, end);
  const uint32_t b = begin - sm.i_begin, e = end - sm.i_begin;
  if (b % tile != 0 || (e % tile != 0 && end != sm.i_end))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                "%s range [%u, %u) is not aligned to the %u-sample tile edge", what,
                begin, end, tile);
  *t0 = b / tile;
  *t1 = (e + tile - 1) / tile;
  return CUKING_OK;
}

cuking_status cuking_prepare_samples(cuking_ctx *ctx, const cuking_submatrix *sm,
                                     uint32_t words_per_sample,
                                     const uint64_t *d_bit_sets,
                                     uint32_t sample_begin, uint32_t sample_end,
                                     void *stream) {
  BIND_OR_RETURN(ctx);
  cuking_status st = check_compute_args(sm, words_per_sample, d_bit_sets);
  if (st != CUKING_OK) return st;
  if (!sm_is_diag(*sm))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                "staged preparation needs a diagonal block (rows == columns)");
  const uint32_t tile = plan_variant(ctx, words_per_sample).tile;
  uint32_t t0, t1;
  st = tile_span(*sm, tile, sample_begin, sample_end, "sample", &t0, &t1);
  if (st != CUKING_OK) return st;
  if (t0 == t1) return CUKING_OK;
  PlaneGeometry geo;
  TileSpace tiles;
  // prepare() works in units of 64 plane samples.  (For the records of rectangles, whatever
  // their threshold: sorted, every code converted, no site order.)
  return prepare(ctx,
                 {*sm, words_per_sample, d_bit_sets, (hipStream_t)stream, t0 * (tile / 64),
                  t1 * (tile / 64), kFormRecords, false, 0.f},
                 &geo, &tiles);
}

cuking_status cuking_compute_king_rect(
    cuking_ctx *ctx, const cuking_submatrix *sm, uint32_t words_per_sample,
    const uint64_t *d_bit_sets, uint32_t row_begin, uint32_t row_end,
    uint32_t row_step, uint32_t col_begin, uint32_t col_end, float kin_threshold,
    uint32_t max_results, cuking_result *d_results, uint32_t *d_result_index,
    uint32_t *d_result_overflow, void *stream) {
  BIND_OR_RETURN(ctx);
  cuking_status st = check_compute_args(sm, words_per_sample, d_bit_sets);
  if (st != CUKING_OK) return st;
  if (!sm_is_diag(*sm))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                "rectangle launches need a diagonal block (rows == columns)");
  if (!d_result_index || !d_result_overflow || (max_results && !d_results))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null result pointer");
  const TiledVariant v = plan_variant(ctx, words_per_sample);
  const PlaneGeometry geo = make_geometry(*sm, words_per_sample, v);
  // Rectangles of a diagonal block contain slots below the diagonal that leave
  // at once; one contiguous chunk of the enumeration per XCD then leaves some
  // XCDs with little real work (100k x 100k in 8 staged rectangles: 0.69 s
  // against 0.63 s round-robin), so rectangles take the XCD order only in its
  // patch form (32 consecutive slots per patch, patches dealt round-robin:
  // 0.66 s), with 17-row bands.
  const TileSpace tiles = make_tiles(geo, v, ctx->band_rows ? ctx->band_rows : 17);
  const size_t need = plane_bytes(geo, v.layout);
  const int variant = effective_variant(ctx, words_per_sample);
  if (ctx->planes == nullptr || ctx->planes_bytes < need ||
      !same_block(ctx->prepared, *sm, words_per_sample, variant, v.tile, d_bit_sets))
    return cuking_fail(CUKING_ERR_FAILED_PRECONDITION,
                "cuking_prepare_samples() has not been called for this block "
                "(or the workspace has been converted for another one since)");
  uint32_t r0, r1, c0, c1;
  st = tile_span(*sm, v.tile, row_begin, row_end, "row", &r0, &r1);
  if (st != CUKING_OK) return st;
  st = tile_span(*sm, v.tile, col_begin, col_end, "column", &c0, &c1);
  if (st != CUKING_OK) return st;
  if (r0 == r1 || c0 == c1) return CUKING_OK;
  if (row_step == 0) row_step = v.tile;
  if (row_step % v.tile != 0)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                "row_step %u is not a multiple of the %u-sample tile edge", row_step,
                v.tile);
  const uint32_t stride = row_step / v.tile;
  const uint32_t n_rows = (r1 - r0 + stride - 1) / stride;
  {
    // Every sample the rectangle reads must have been converted.
    const uint32_t per = v.tile / 64;
    const std::vector<uint8_t> &done = ctx->prepared.tiles;
    auto converted = [&](uint32_t tile) {
      for (uint32_t t = tile * per; t < (tile + 1) * per; ++t)
        if (t >= done.size() || !done[t]) return false;
      return true;
    };
    for (uint32_t r = r0; r < r1; r += stride)
      if (!converted(r))
        return cuking_fail(CUKING_ERR_FAILED_PRECONDITION,
                    "row samples from %u on have not been prepared",
                    sm->i_begin + r * v.tile);
    for (uint32_t c = c0; c < c1; ++c)
      if (!converted(c))
        return cuking_fail(CUKING_ERR_FAILED_PRECONDITION,
                    "column samples from %u on have not been prepared",
                    sm->i_begin + c * v.tile);
  }

  const bool full = use_full_counts(ctx, kin_threshold, words_per_sample);
  LaunchSwitches sw = launch_switches(ctx, words_per_sample, kFormRecords, full, kin_threshold);
  TiledArgs a;
  st = launch_args(ctx, (hipStream_t)stream, *sm, words_per_sample, d_bit_sets, geo, tiles,
                   total_tiles(make_tiles(geo, v, ctx->band_rows)),
                   record_outputs(kFormRecords, kin_threshold, max_results, d_results,
                                  d_result_index, d_result_overflow),
                   &a);
  if (st != CUKING_OK) return st;
  a.rect_rows = n_rows;
  a.rect_cols = c1 - c0;
  a.rect_row0 = r0;
  a.rect_col0 = c0;
  a.rect_row_stride = stride;
  if (sw.xcd_swizzle != 2) sw.xcd_swizzle = 0;  // (see above; patches keep the balance)
  if (v.layout == kLayoutNibbleStats && !ctx->prepared.codes && !sw.filter_runs) {
    // (a block converted without the four-product kernel's codes, and a call that runs
    //  that kernel directly)
    st = convert_codes_now(ctx, geo, words_per_sample, d_bit_sets, (hipStream_t)stream);
    if (st != CUKING_OK) return st;
    a.codes_ready = nullptr;
  }
  EventPair *ev = nullptr;
  if (ctx->timing) HIP_TRY(ctx->king_timer.begin((hipStream_t)stream, &ev));
  HIP_TRY(launch_planned(ctx, words_per_sample, full, a, sw, (uint64_t)n_rows * (c1 - c0),
                         (hipStream_t)stream));
  note_reader(ctx, (hipStream_t)stream);
  {
    const uint32_t per = v.tile / 64;
    for (uint32_t r = r0; r < r1; r += stride) mark_read(ctx, r * per, (r + 1) * per);
    mark_read(ctx, c0 * per, c1 * per);
  }
  if (ev) HIP_TRY(hipEventRecord(ev->stop, (hipStream_t)stream));
  return CUKING_OK;
}

cuking_status cuking_ctx_reserve(cuking_ctx *ctx, const cuking_submatrix *sm,
                                 uint32_t words_per_sample, void *const *streams,
                                 size_t num_streams) {
  BIND_OR_RETURN(ctx);
  cuking_status st = cuking_check_block(sm, words_per_sample);
  if (st != CUKING_OK) return st;
  if (num_streams != 0 && streams == nullptr)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null stream list");
  if (sm_num_rows(*sm) == 0 || sm_num_cols(*sm) == 0) return CUKING_OK;
  const TiledVariant v = plan_variant(ctx, words_per_sample);
  const PlaneGeometry geo = make_geometry(*sm, words_per_sample, v);
  const TileSpace tiles = make_tiles(geo, v, ctx->band_rows);
  st = ensure_workspace(ctx, geo, v, tiles);
  if (st != CUKING_OK) return st;
  if (!same_tile_space(ctx->prefix_for, tiles)) {
    // (nothing may be reading another block's prefix: the caller reserves
    //  before it enqueues work for this block)
    if (!ctx->readers.empty()) {
      ++ctx->host_syncs;
      HIP_TRY(hipDeviceSynchronize());
    }
    st = upload_prefix(ctx, tiles, nullptr);
    if (st != CUKING_OK) return st;
  }
  if (num_streams > kMaxStreams)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "at most %zu streams per context can be reserved", kMaxStreams);
  auto named = [&](hipStream_t s) {
    for (size_t k = 0; k < num_streams; ++k)
      if ((hipStream_t)streams[k] == s) return true;
    return false;
  };
  if (uses_split_slab(ctx) || uses_filter_scratch(ctx)) {
    // Make room now, so that no stream reserved here is the one evicted for a later one:
    // the oldest entries this reservation does not name go.
    size_t missing = num_streams;
    for (const auto &e : ctx->scratch) missing -= named(e.stream) ? 1 : 0;
    for (size_t k = 0; ctx->scratch.size() + missing > kMaxStreams;) {
      if (named(ctx->scratch[k].stream))
        ++k;
      else
        evict_scratch(ctx, k);
    }
  }
  for (size_t k = 0; k < num_streams; ++k) {
    cuking_ctx::StreamScratch *e;
    st = scratch_for(ctx, (hipStream_t)streams[k], total_tiles(tiles), &e);
    if (st != CUKING_OK) return st;
  }
  return CUKING_OK;
}

cuking_status cuking_invalidate(cuking_ctx *ctx) {
  if (ctx == nullptr) return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null context");
  // The next conversion treats the workspace as another block's: it is ordered
  // behind every kernel that may still read it.
  ctx->prepared.valid = false;
  return CUKING_OK;
}

cuking_status cuking_compute_counts(cuking_ctx *ctx, const cuking_submatrix *sm,
                                    uint32_t words_per_sample,
                                    const uint64_t *d_bit_sets,
                                    cuking_counts *d_counts, void *stream) {
  BIND_OR_RETURN(ctx);
  cuking_status st = check_compute_args(sm, words_per_sample, d_bit_sets);
  if (st != CUKING_OK) return st;
  if (sm_num_rows(*sm) == 0 || sm_num_cols(*sm) == 0) return CUKING_OK;
  if (d_counts == nullptr)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null counts pointer");
  const BlockArgs b = {ctx, sm, words_per_sample, d_bit_sets, stream};
  Outputs out = {};
  out.form = kFormCounts;
  out.counts = d_counts;
  return ctx->kernel == CUKING_KERNEL_STREAM ? run_stream(b, out) : run_tiled(b, kEveryTile, out);
}

// cuking_compute_kin_matrix and cuking_compute_kin_matrix_tiles.  (Every check in front of
// anything that touches a device, the null context last among them; then the device is bound,
// an empty block or not.)
static cuking_status kin_matrix_call(const BlockArgs &b, const TileRange &r, float *d_kin,
                                     uint64_t ld, uint32_t flags) {
  return run_pair_call(b, r, BindAt::kBehindCheck, [&](Outputs *out) {
    const cuking_submatrix *sm = b.sm;
    const cuking_status st = check_compute_args(sm, b.words_per_sample, b.d_bit_sets);
    if (st != CUKING_OK) return st;
    if (flags != CUKING_KIN_UPPER && flags != CUKING_KIN_SYMMETRIC)
      return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "unknown kinship matrix flags 0x%x", flags);
    if (ld < sm_num_cols(*sm))
      return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                         "kinship matrix: leading dimension %llu below the block's %u columns",
                         (unsigned long long)ld, sm_num_cols(*sm));
    if (flags == CUKING_KIN_SYMMETRIC && !sm_is_diag(*sm))
      return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                         "a symmetric kinship matrix needs a diagonal block (rows == columns)");
    if (flags == CUKING_KIN_SYMMETRIC && !r.whole)
      return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                         "a symmetric kinship matrix cannot be computed by tile ranges");
    if (sm_num_rows(*sm) != 0 && sm_num_cols(*sm) != 0 && d_kin == nullptr)
      return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null kinship matrix pointer");
    if (b.ctx == nullptr) return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null context");
    out->form = kFormKinMatrix;
    out->kin = d_kin;
    out->kin_ld = ld;
    out->kin_flags = flags;
    return CUKING_OK;
  });
}

cuking_status cuking_compute_kin_matrix(cuking_ctx *ctx, const cuking_submatrix *sm,
                                        uint32_t words_per_sample, const uint64_t *d_bit_sets,
                                        float *d_kin, uint64_t ld, uint32_t flags,
                                        void *stream) {
  return kin_matrix_call({ctx, sm, words_per_sample, d_bit_sets, stream}, kEveryTile, d_kin, ld,
                         flags);
}

cuking_status cuking_compute_kin_matrix_tiles(cuking_ctx *ctx, const cuking_submatrix *sm,
                                              uint32_t words_per_sample,
                                              const uint64_t *d_bit_sets, uint64_t tile_begin,
                                              uint64_t tile_end, float *d_kin, uint64_t ld,
                                              uint32_t flags, void *stream) {
  return kin_matrix_call({ctx, sm, words_per_sample, d_bit_sets, stream},
                         {false, tile_begin, tile_end}, d_kin, ld, flags);
}

// What the checks of the matrix-core-only calls (kinship summary, relative counts, PI_HAT)
// end with, in front of anything that touches a device: the tile range, the context and what
// it can serve.  `what` names the call, `form` the kernel form a context may lack.
static cuking_status check_reducing_args(const BlockArgs &b, const TileRange &r, const char *what,
                                         const char *form) {
  const cuking_ctx *ctx = b.ctx;
  if (!r.whole && r.begin > r.end)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "tile range [%llu, %llu) is reversed",
                       (unsigned long long)r.begin, (unsigned long long)r.end);
  if (ctx == nullptr) return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null context");
  // (run_tiled checks the range as well, but only behind the conversion: this call refuses
  //  a bad range before a device is touched)
  if (!r.whole) {
    const bool empty = sm_num_rows(*b.sm) == 0 || sm_num_cols(*b.sm) == 0;
    const uint64_t n_tiles = empty ? 0 : cuking_num_tiles(ctx, b.sm);
    if (r.end > n_tiles)
      return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "tile range [%llu, %llu) outside [0, %llu)",
                         (unsigned long long)r.begin, (unsigned long long)r.end,
                         (unsigned long long)n_tiles);
  }
  if (ctx->kernel != CUKING_KERNEL_TILED || !is_mfma_variant(ctx->variant))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "%s: served by contexts of the tiled kernel with variant 5, 6 or 7 (the "
                       "matrix-core kernels) only; the VALU variants and the stream kernel have "
                       "no %s", what, form);
  if (!is_mfma_variant(effective_variant(ctx, b.words_per_sample)))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "%s: bitsets from 2^24 sites on are not served (the matrix-core kernels "
                       "count in float32)", what);
  return CUKING_OK;
}

// cuking_compute_kin_summary and cuking_compute_kin_summary_tiles.  (This call and the two
// below: every check in front of anything that touches a device; an empty block returns
// before the device is bound.)
static cuking_status kin_summary_call(const BlockArgs &b, const TileRange &r,
                                      const cuking_kin_bins *bins, uint64_t *d_hist,
                                      uint64_t *d_best) {
  return run_pair_call(b, r, BindAt::kBehindEmptyBlock, [&](Outputs *out) {
    const cuking_status st = check_compute_args(b.sm, b.words_per_sample, b.d_bit_sets);
    if (st != CUKING_OK) return st;
    if (d_hist == nullptr && d_best == nullptr)
      return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                         "kinship summary: both outputs (histogram and nearest relatives) are null");
    if (d_hist != nullptr) {
      if (bins == nullptr)
        return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                           "kinship summary: a histogram needs bins (null bins pointer)");
      if (bins->num_bins == 0 || bins->num_bins > CUKING_KIN_BINS_MAX)
        return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                           "kinship summary: num_bins %u outside [1, %u]", bins->num_bins,
                           CUKING_KIN_BINS_MAX);
      if (!kin_bins_valid(*bins))
        return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                           "kinship summary: histogram bounds must be finite with lo < hi "
                           "(lo %g, hi %g)", (double)bins->lo, (double)bins->hi);
      out->sum_bins = *bins;
    }
    out->form = kFormKinSummary;
    out->sum_hist = d_hist;
    out->sum_best = d_best;
    return check_reducing_args(b, r, "kinship summary", "summary form");
  });
}

cuking_status cuking_compute_kin_summary(cuking_ctx *ctx, const cuking_submatrix *sm,
                                         uint32_t words_per_sample, const uint64_t *d_bit_sets,
                                         const cuking_kin_bins *bins, uint64_t *d_hist,
                                         uint64_t *d_best, void *stream) {
  return kin_summary_call({ctx, sm, words_per_sample, d_bit_sets, stream}, kEveryTile, bins,
                          d_hist, d_best);
}

cuking_status cuking_compute_kin_summary_tiles(cuking_ctx *ctx, const cuking_submatrix *sm,
                                               uint32_t words_per_sample,
                                               const uint64_t *d_bit_sets, uint64_t tile_begin,
                                               uint64_t tile_end, const cuking_kin_bins *bins,
                                               uint64_t *d_hist, uint64_t *d_best,
                                               void *stream) {
  return kin_summary_call({ctx, sm, words_per_sample, d_bit_sets, stream},
                          {false, tile_begin, tile_end}, bins, d_hist, d_best);
}

// cuking_compute_relative_counts and cuking_compute_relative_counts_tiles.
static cuking_status relative_counts_call(const BlockArgs &b, const TileRange &r,
                                          const float *thresholds, uint32_t num_thresholds,
                                          uint32_t *d_counts) {
  return run_pair_call(b, r, BindAt::kBehindEmptyBlock, [&](Outputs *out) {
    const cuking_status st = check_compute_args(b.sm, b.words_per_sample, b.d_bit_sets);
    if (st != CUKING_OK) return st;
    if (thresholds == nullptr)
      return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "relative counts: null thresholds pointer");
    if (num_thresholds == 0 || num_thresholds > CUKING_REL_THRESHOLDS_MAX)
      return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                         "relative counts: num_thresholds %u outside [1, %u]", num_thresholds,
                         CUKING_REL_THRESHOLDS_MAX);
    if (!rel_thresholds_valid(thresholds, num_thresholds))
      return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                         "relative counts: thresholds must be finite and strictly ascending");
    if (sm_num_samples(*b.sm) != 0 && d_counts == nullptr)
      return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "relative counts: null counts pointer");
    out->form = kFormRelCounts;
    out->kin_threshold = thresholds[0];
    out->rel_counts = d_counts;
    out->rel_num = num_thresholds;
    for (uint32_t t = 0; t < num_thresholds; ++t) out->rel_thr[t] = thresholds[t];
    return check_reducing_args(b, r, "relative counts", "counting form");
  });
}

cuking_status cuking_compute_relative_counts(cuking_ctx *ctx, const cuking_submatrix *sm,
                                             uint32_t words_per_sample,
                                             const uint64_t *d_bit_sets, const float *thresholds,
                                             uint32_t num_thresholds, uint32_t *d_counts,
                                             void *stream) {
  return relative_counts_call({ctx, sm, words_per_sample, d_bit_sets, stream}, kEveryTile,
                              thresholds, num_thresholds, d_counts);
}

cuking_status cuking_compute_relative_counts_tiles(cuking_ctx *ctx, const cuking_submatrix *sm,
                                                   uint32_t words_per_sample,
                                                   const uint64_t *d_bit_sets, uint64_t tile_begin,
                                                   uint64_t tile_end, const float *thresholds,
                                                   uint32_t num_thresholds, uint32_t *d_counts,
                                                   void *stream) {
  return relative_counts_call({ctx, sm, words_per_sample, d_bit_sets, stream},
                              {false, tile_begin, tile_end}, thresholds, num_thresholds, d_counts);
}

// ---- PI_HAT records (king_pihat.h) ----------------------------------------------------------

// cuking_compute_pihat and cuking_compute_pihat_tiles: the thresholded call's route at
// threshold 0 (every tile, no filter) with the PI_HAT form.
static cuking_status pihat_call(const BlockArgs &b, const TileRange &r,
                                const cuking_pihat_model *model, float min_pi_hat, uint32_t flags,
                                uint32_t max_results, cuking_result *d_results,
                                uint32_t *d_result_index, uint32_t *d_result_overflow) {
  return run_pair_call(b, r, BindAt::kBehindEmptyBlock, [&](Outputs *out) {
    cuking_status st = check_compute_args(b.sm, b.words_per_sample, b.d_bit_sets);
    if (st != CUKING_OK) return st;
    st = cuking_check_pihat_args(model, flags);
    if (st != CUKING_OK) return st;
    if (!d_result_index || !d_result_overflow || (max_results && !d_results))
      return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null result pointer");
    *out = record_outputs(kFormPiHat, 0.f, max_results, d_results, d_result_index,
                          d_result_overflow);
    out->pihat = PihatArgs{model->e00, model->e01, model->e02, model->e11, model->e12,
                           min_pi_hat, flags, 1u};
    return check_reducing_args(b, r, "pi_hat", "PI_HAT form");
  });
}

cuking_status cuking_compute_pihat(cuking_ctx *ctx, const cuking_submatrix *sm,
                                   uint32_t words_per_sample, const uint64_t *d_bit_sets,
                                   const cuking_pihat_model *model, float min_pi_hat,
                                   uint32_t flags, uint32_t max_results, cuking_result *d_results,
                                   uint32_t *d_result_index, uint32_t *d_result_overflow,
                                   void *stream) {
  return pihat_call({ctx, sm, words_per_sample, d_bit_sets, stream}, kEveryTile, model,
                    min_pi_hat, flags, max_results, d_results, d_result_index, d_result_overflow);
}

cuking_status cuking_compute_pihat_tiles(cuking_ctx *ctx, const cuking_submatrix *sm,
                                         uint32_t words_per_sample, const uint64_t *d_bit_sets,
                                         uint64_t tile_begin, uint64_t tile_end,
                                         const cuking_pihat_model *model, float min_pi_hat,
                                         uint32_t flags, uint32_t max_results,
                                         cuking_result *d_results, uint32_t *d_result_index,
                                         uint32_t *d_result_overflow, void *stream) {
  return pihat_call({ctx, sm, words_per_sample, d_bit_sets, stream},
                    {false, tile_begin, tile_end}, model, min_pi_hat, flags, max_results,
                    d_results, d_result_index, d_result_overflow);
}

// ---- unrelated set and families from the records (king_unrelated.h, king_prune.hip) --------

cuking_status cuking_unrelated_set(cuking_ctx *ctx, const cuking_result *d_records,
                                   uint64_t num_records, uint32_t num_samples,
                                   float prune_threshold, const float *d_priority,
                                   uint8_t *d_keep, uint32_t *d_family, uint32_t *rounds,
                                   void *stream) {
  if (rounds != nullptr) *rounds = 0;
  if (ctx == nullptr) return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null context");
  if (!unrel_threshold_valid(prune_threshold))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "unrelated set: prune_threshold is NaN");
  if (num_records != 0 && d_records == nullptr)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "unrelated set: null records pointer");
  if (num_samples != 0 && d_keep == nullptr)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "unrelated set: null keep pointer");
  if (num_samples > kUnrelMaxSamples || num_records > kUnrelMaxRecords)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "unrelated set: at most 2^31 samples and 2^30 records are served");
  if (num_samples == 0 && num_records != 0)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "unrelated set: records name samples outside [0, num_samples)");
  if (num_samples == 0) return CUKING_OK;
  BIND_OR_RETURN(ctx);
  // The stream's entry of the scratch cache; the workspace is sized once per call, in front
  // of the round loop, and grown only when a call needs more.
  hipStream_t s = (hipStream_t)stream;
  cuking_ctx::StreamScratch *e = stream_entry(ctx, s);
  const size_t bytes = prune_workspace_bytes((uint32_t)num_records, num_samples,
                                             d_priority == nullptr);
  const cuking_status st = grow_on_stream(ctx, s, &e->prune, bytes);
  if (st != CUKING_OK) return st;
  uint32_t done = 0, syncs = 0;
  int invalid = 0, exceeded = 0;
  const int err = prune_run(e->prune.p, d_records, (uint32_t)num_records, num_samples,
                            prune_threshold, d_priority, d_keep, d_family, ctx->num_cus, &done,
                            &syncs, &invalid, &exceeded, stream);
  ctx->host_syncs += syncs;
  if (err != 0) {
    (void)hipGetLastError();
    return cuking_fail((hipError_t)err == hipErrorOutOfMemory ? CUKING_ERR_OUT_OF_MEMORY
                                                              : CUKING_ERR_DEVICE,
                       "unrelated set: %s", hipGetErrorString((hipError_t)err));
  }
  if (invalid)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "unrelated set: a record does not satisfy sample_i < sample_j < "
                       "num_samples (%u)", num_samples);
  if (exceeded)
    return cuking_fail(CUKING_ERR_DEVICE,
                       "unrelated set: internal error, a loop ran past its bound of %u rounds",
                       num_samples);
  if (rounds != nullptr) *rounds = done;
  return CUKING_OK;
}

// ---- site QC (king_site_qc.hip) -------------------------------------------

cuking_status cuking_site_counts(cuking_ctx *ctx, const uint64_t *d_bit_set,
                                 uint32_t num_stored, uint32_t words_per_sample,
                                 uint32_t *d_counts, void *stream) {
  // (the arguments first: a refused call touches no device)
  if (ctx == nullptr) return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null context");
  cuking_status st = cuking_check_counts_args("site counts", d_bit_set, num_stored,
                                              words_per_sample, d_counts);
  if (st != CUKING_OK) return st;
  if (num_stored == 0) return CUKING_OK;
  BIND_OR_RETURN(ctx);
  HIP_TRY(launch_site_counts(d_bit_set, num_stored, words_per_sample, d_counts,
                             (hipStream_t)stream));
  return CUKING_OK;
}

cuking_status cuking_test_site_gather(cuking_ctx *ctx, const uint64_t *d_bit_set,
                                      uint32_t num_stored, uint32_t words_per_sample,
                                      const uint32_t *d_order, int gather, uint64_t *d_permuted,
                                      int stats, void *d_stats, uint64_t stats_bytes,
                                      uint64_t *layout, void *stream) {
  if (ctx == nullptr) return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null context");
  if (d_bit_set == nullptr || d_order == nullptr || d_permuted == nullptr)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "site gather: null pointer");
  if (num_stored == 0 || words_per_sample < 2)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "site gather: no samples or no plane words");
  if ((gather != 0 && gather != 2 && gather != 4) ||
      site_gather_pick(gather, words_per_sample) != gather)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "site gather: form %d does not serve %u words per sample", gather,
                       words_per_sample);
  if (stats < 0 || stats > 2 || (stats == 1 && gather == 0))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "site gather: statistics %d with form %d (0 none, 1 inside the byte-wide "
                       "gather, 2 the separate kernel)", stats, gather);
  // The statistics of a whole diagonal block of num_stored samples in the filter variant's
  // geometry: stats, cum, the sums and the check steps one behind the other.
  cuking_submatrix sm;
  cuking_status status = cuking_submatrix_init(&sm, num_stored, 1, 0);
  if (status != CUKING_OK) return status;
  const PlaneGeometry geo = make_geometry(sm, words_per_sample, tiled_variant(7));
  const uint64_t off_cum = (uint64_t)geo.s_stride * sizeof(float2);
  const uint64_t off_sums = off_cum + (uint64_t)geo.s_stride * (kNumCum + 1) * sizeof(float);
  const uint64_t off_steps = off_sums + 64, bytes = off_steps + 64;
  if (layout != nullptr) {
    layout[0] = geo.s_stride;
    layout[1] = off_cum;
    layout[2] = off_sums;
    layout[3] = off_steps;
    layout[4] = bytes;
  }
  if (stats != 0 && (d_stats == nullptr || stats_bytes < bytes))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "site gather: the statistics need %llu bytes", (unsigned long long)bytes);
  BIND_OR_RETURN(ctx);
  uint8_t *base = static_cast<uint8_t *>(d_stats);
  SiteGatherStats fused = {};
  if (stats != 0) {
    fused.to = {reinterpret_cast<float2 *>(base), reinterpret_cast<float *>(base + off_cum),
                reinterpret_cast<unsigned long long *>(base + off_sums),
                reinterpret_cast<uint32_t *>(base + off_steps)};
    fused.geo = geo;
    fused.s_end = geo.s_stride;
    HIP_TRY(hipMemsetAsync(base + off_sums, 0, 64, (hipStream_t)stream));
  }
  HIP_TRY(launch_site_gather(d_bit_set, num_stored, words_per_sample, d_order, d_permuted, gather,
                             stats == 1 ? &fused : nullptr, (hipStream_t)stream));
  // (the padding samples behind the stored ones, or with 2 every plane sample, as prepare())
  if (stats != 0)
    HIP_TRY(launch_sample_stats_to(d_permuted, words_per_sample, geo, fused.to,
                                   stats == 1 ? num_stored : 0, geo.s_stride,
                                   (hipStream_t)stream));
  return CUKING_OK;
}

cuking_status cuking_sample_counts(cuking_ctx *ctx, const uint64_t *d_bit_set,
                                   uint32_t num_stored, uint32_t words_per_sample,
                                   uint32_t num_sites, uint32_t *d_counts, void *stream) {
  if (ctx == nullptr) return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null context");
  cuking_status st = cuking_check_counts_args("sample counts", d_bit_set, num_stored,
                                              words_per_sample, d_counts);
  if (st != CUKING_OK) return st;
  if (cuking_words_per_sample(num_sites) != words_per_sample)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "sample counts: %u sites need %u words per sample, not %u", num_sites,
                       cuking_words_per_sample(num_sites), words_per_sample);
  if (num_stored == 0) return CUKING_OK;
  BIND_OR_RETURN(ctx);
  HIP_TRY(launch_sample_counts(d_bit_set, num_stored, words_per_sample, num_sites, d_counts,
                               (hipStream_t)stream));
  return CUKING_OK;
}

cuking_status cuking_compact_sites(cuking_ctx *ctx, const uint64_t *d_in, uint32_t num_stored,
                                   uint32_t words_per_sample_in, const uint64_t *keep,
                                   uint32_t num_sites_in, uint64_t *d_out,
                                   uint32_t words_per_sample_out, void *stream) {
  if (ctx == nullptr) return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null context");
  uint32_t kept = 0;
  cuking_status st = cuking_check_compact_args(d_in, num_stored, words_per_sample_in, keep,
                                               num_sites_in, d_out, words_per_sample_out, &kept);
  if (st != CUKING_OK) return st;
  if (num_stored == 0) return CUKING_OK;
  BIND_OR_RETURN(ctx);
  hipStream_t s = (hipStream_t)stream;
  cuking_ctx::StreamScratch *e = stream_entry(ctx, s);
  const uint32_t plane_in = words_per_sample_in / 2, plane_out = words_per_sample_out / 2;
  const size_t bytes = compact_table_bytes(plane_in, plane_out);
  st = grow_on_stream(ctx, s, &e->sites, bytes);
  if (st != CUKING_OK) return st;
  // (8-byte units: the table starts with uint64 fields)
  std::vector<uint64_t> table((bytes + 7) / 8);
  build_compact_table(keep, plane_in, plane_out, table.data());
  // Ordered on the stream behind whatever still reads the table of an earlier call.  Small and
  // pageable: wait until the host buffer may go away.
  HIP_TRY(hipMemcpyAsync(e->sites.p, table.data(), bytes, hipMemcpyHostToDevice, s));
  ++ctx->host_syncs;
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(launch_compact_sites(d_in, num_stored, words_per_sample_in, e->sites.p, kept, d_out,
                               words_per_sample_out, s));
  return CUKING_OK;
}

// ---- LD pruning (king_ld.hip) ----------------------------------------------

cuking_status cuking_transpose_sites(cuking_ctx *ctx, const uint64_t *d_bit_set,
                                     uint32_t num_stored, uint32_t words_per_sample,
                                     uint32_t num_sites, uint64_t *d_site_bits,
                                     uint32_t words_per_site_plane, void *stream) {
  if (ctx == nullptr) return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null context");
  cuking_status st = cuking_check_transpose_args(d_bit_set, num_stored, words_per_sample,
                                                 num_sites, d_site_bits, words_per_site_plane);
  if (st != CUKING_OK) return st;
  if (num_stored == 0 || num_sites == 0) return CUKING_OK;
  BIND_OR_RETURN(ctx);
  HIP_TRY(launch_transpose_sites(d_bit_set, num_stored, words_per_sample, num_sites, d_site_bits,
                                 (hipStream_t)stream));
  return CUKING_OK;
}

cuking_status cuking_ld_edges(cuking_ctx *ctx, const uint64_t *d_site_bits, uint32_t num_sites,
                              uint32_t num_stored, uint32_t window, float r2_threshold,
                              const int32_t *d_group, cuking_result *d_records,
                              uint64_t max_records, uint64_t *num_records, void *stream) {
  if (num_records != nullptr) *num_records = 0;
  if (ctx == nullptr) return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null context");
  cuking_status st = cuking_check_ld_args(d_site_bits, num_stored, window, r2_threshold,
                                          d_records, max_records, num_records);
  if (st != CUKING_OK) return st;
  if (num_sites < 2 || num_stored == 0) return CUKING_OK;
  BIND_OR_RETURN(ctx);
  return counted_output(ctx, (hipStream_t)stream, max_records, num_records, cuking_ld_count_status,
                        [&](unsigned long long *d_count, hipStream_t s) {
                          return launch_ld_edges(d_site_bits, num_sites, num_stored, window,
                                                 r2_threshold, d_group, d_records, max_records,
                                                 d_count, s);
                        });
}

// ---- genotype matrix products (king_geno.hip) -------------------------------

cuking_status cuking_geno_matmul(cuking_ctx *ctx, const uint64_t *d_bits, uint32_t num_rows,
                                 uint32_t words_per_row, uint32_t num_cols, const float *d_table,
                                 int table_axis, const float *d_b, uint32_t ldb, uint32_t num_rhs,
                                 float *d_out, uint32_t ldo, void *stream) {
  // (the arguments first: a refused call touches no device)
  if (ctx == nullptr) return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null context");
  const cuking_status st = cuking_check_geno_args(d_bits, num_rows, words_per_row, num_cols,
                                                  d_table, table_axis, d_b, ldb, num_rhs, d_out,
                                                  ldo);
  if (st != CUKING_OK) return st;
  if (num_rows == 0) return CUKING_OK;
  BIND_OR_RETURN(ctx);
  HIP_TRY(launch_geno_matmul(d_bits, num_rows, words_per_row, num_cols, d_table,
                             table_axis == kGenoTablePerRow, d_b, ldb, num_rhs, d_out, ldo,
                             (hipStream_t)stream));
  return CUKING_OK;
}

// ---- PC-Relate (king_pcrelate.hip) -------------------------------------------

cuking_status cuking_pcrelate_matrix(cuking_ctx *ctx, const uint64_t *d_bits, uint32_t num_stored,
                                     uint32_t words_per_sample, uint32_t num_sites,
                                     const float *d_x, uint32_t ldx, const float *d_beta,
                                     uint32_t ldbeta, uint32_t d, float lo, float hi,
                                     const cuking_submatrix *block, float *d_out, uint64_t ldo,
                                     void *stream) {
  // (the arguments first: a refused call touches no device)
  if (ctx == nullptr) return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null context");
  const cuking_status st = cuking_check_pcrelate_args(d_bits, num_stored, words_per_sample,
                                                      num_sites, d_x, ldx, d_beta, ldbeta, d, lo,
                                                      hi, block, d_out, ldo);
  if (st != CUKING_OK) return st;
  if (sm_num_rows(*block) == 0 || sm_num_cols(*block) == 0) return CUKING_OK;
  BIND_OR_RETURN(ctx);
  HIP_TRY(launch_pcrelate_matrix(d_bits, words_per_sample, num_sites, d_x, ldx, d_beta, ldbeta, d,
                                 lo, hi, *block, d_out, ldo, (hipStream_t)stream));
  return CUKING_OK;
}

cuking_status cuking_pcrelate_records(cuking_ctx *ctx, const uint64_t *d_bits,
                                      uint32_t num_stored, uint32_t words_per_sample,
                                      uint32_t num_sites, const float *d_x, uint32_t ldx,
                                      const float *d_beta, uint32_t ldbeta, uint32_t d, float lo,
                                      float hi, const cuking_submatrix *block, float min_kin,
                                      cuking_result *d_records, uint64_t max_records,
                                      uint64_t *num_records, void *stream) {
  if (num_records != nullptr) *num_records = 0;
  // (the arguments first: a refused call touches no device)
  if (ctx == nullptr) return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null context");
  cuking_status st = cuking_check_pcrelate_records_args(
      d_bits, num_stored, words_per_sample, num_sites, d_x, ldx, d_beta, ldbeta, d, lo, hi, block,
      min_kin, d_records, max_records, num_records);
  if (st != CUKING_OK) return st;
  // (without a site every kin is NaN: no record)
  if (sm_num_rows(*block) == 0 || sm_num_cols(*block) == 0 || num_sites == 0) return CUKING_OK;
  BIND_OR_RETURN(ctx);
  return counted_output(
      ctx, (hipStream_t)stream, max_records, num_records, cuking_pcrelate_count_status,
      [&](unsigned long long *d_count, hipStream_t s) {
        return launch_pcrelate_records(d_bits, words_per_sample, num_sites, d_x, ldx, d_beta,
                                       ldbeta, d, lo, hi, *block, min_kin, d_records, max_records,
                                       d_count, s);
      });
}

cuking_status cuking_pcrelate_pairs(cuking_ctx *ctx, const uint64_t *d_bits, uint32_t num_stored,
                                    uint32_t words_per_sample, uint32_t num_sites,
                                    const float *d_x, uint32_t ldx, const float *d_beta,
                                    uint32_t ldbeta, uint32_t d, float lo, float hi,
                                    const float *d_f, const void *d_pairs, uint64_t num_pairs,
                                    uint32_t pair_stride, cuking_pcrelate_pair *d_out,
                                    void *stream) {
  // (the arguments first: a refused call touches no device)
  if (ctx == nullptr) return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null context");
  const cuking_status st = cuking_check_pcrelate_pairs_args(d_bits, words_per_sample, num_sites,
                                                            d_x, ldx, d_beta, ldbeta, d, lo, hi,
                                                            d_pairs, num_pairs, pair_stride, d_out);
  if (st != CUKING_OK) return st;
  if (num_pairs == 0) return CUKING_OK;
  BIND_OR_RETURN(ctx);
  HIP_TRY(launch_pcrelate_pairs(d_bits, num_stored, words_per_sample, num_sites, d_x, ldx, d_beta,
                                ldbeta, d, lo, hi, d_f, d_pairs, num_pairs, pair_stride, d_out,
                                (hipStream_t)stream));
  return CUKING_OK;
}

// ---- IBD segments for listed pairs (king_ibd.hip) ------------------------------

// What the pair calls and the scan of single samples share once their arguments are checked and
// there is work to do: the host check of the positions, the group bits of the stream's scratch
// and `launch(d_group_bits, d_count, stream)` -- as a counted output judged by `count_status`
// (segments for the listed calls, records for the scan of a block) when a count is wanted.
extern "C++" {
template <class Launch>
static cuking_status ibd_scan_device(cuking_ctx *ctx, uint32_t num_sites, const int32_t *d_group,
                                     const uint32_t *d_pos, uint64_t max_segments,
                                     uint64_t *num_segments, void *stream, Launch &&launch,
                                     cuking_status (*count_status)(uint64_t, uint64_t) =
                                         cuking_ibd_count_status) {
  BIND_OR_RETURN(ctx);
  hipStream_t s = (hipStream_t)stream;
  cuking_status st;
  if (d_pos != nullptr && num_sites > 1) {
    // The host check of the positions, on copies: ordered on the stream behind whatever
    // writes the arrays.
    std::vector<uint32_t> pos(num_sites);
    std::vector<int32_t> group(d_group != nullptr ? num_sites : 0);
    HIP_TRY(hipMemcpyAsync(pos.data(), d_pos, (size_t)num_sites * 4, hipMemcpyDeviceToHost, s));
    if (d_group != nullptr)
      HIP_TRY(hipMemcpyAsync(group.data(), d_group, (size_t)num_sites * 4,
                             hipMemcpyDeviceToHost, s));
    ++ctx->host_syncs;
    HIP_TRY(hipStreamSynchronize(s));
    st = cuking_check_ibd_positions(d_group != nullptr ? group.data() : nullptr, pos.data(),
                                    num_sites);
    if (st != CUKING_OK) return st;
  }
  cuking_ctx::StreamScratch *e = stream_entry(ctx, s);
  st = grow_on_stream(ctx, s, &e->ibd_groups, ibd_scan_words(num_sites) * sizeof(uint64_t));
  if (st != CUKING_OK) return st;
  uint64_t *d_group_bits = static_cast<uint64_t *>(e->ibd_groups.p);
  HIP_TRY(launch_ibd_group_bits(d_group, num_sites, d_group_bits, s));
  if (num_segments == nullptr) {  // no count wanted: nothing to wait for
    HIP_TRY(launch(d_group_bits, nullptr, s));
    return CUKING_OK;
  }
  return counted_output(ctx, s, max_segments, num_segments, count_status,
                        [&](unsigned long long *d_count, hipStream_t on) {
                          return launch(d_group_bits, d_count, on);
                        });
}
}  // extern "C++"

// Both entry points: bridge_sites == 0 is the strict call.
static cuking_status ibd_pairs_device(cuking_ctx *ctx, const uint64_t *d_bits,
                                      uint32_t num_stored, uint32_t words_per_sample,
                                      uint32_t num_sites, const int32_t *d_group,
                                      const uint32_t *d_pos, uint32_t min_sites,
                                      uint32_t min_length, uint32_t bridge_sites,
                                      const void *d_pairs, uint64_t num_pairs,
                                      uint32_t pair_stride, cuking_ibd_pair *d_out,
                                      uint32_t *d_bridged, cuking_ibd_segment *d_segments,
                                      uint64_t max_segments, uint64_t *num_segments,
                                      void *stream) {
  if (num_segments != nullptr) *num_segments = 0;
  // (the arguments first: a refused call touches no device)
  if (ctx == nullptr) return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null context");
  cuking_status st = cuking_check_ibd_args(d_bits, words_per_sample, num_sites, min_sites,
                                           d_pairs, num_pairs, pair_stride, d_out, d_segments,
                                           max_segments, num_segments);
  if (st != CUKING_OK) return st;
  st = cuking_check_ibd_bridge(bridge_sites);
  if (st != CUKING_OK) return st;
  if (num_pairs == 0) return CUKING_OK;
  return ibd_scan_device(
      ctx, num_sites, d_group, d_pos, max_segments, num_segments, stream,
      [&](const uint64_t *d_group_bits, unsigned long long *d_count, hipStream_t s) {
        return launch_ibd_pairs(d_bits, num_stored, words_per_sample, num_sites, d_group_bits,
                                d_pos, min_sites, min_length, bridge_sites, d_pairs, num_pairs,
                                pair_stride, d_out, d_bridged, d_segments, max_segments, d_count,
                                s);
      });
}

// ---- runs of homozygosity (king_ibd.hip) ----------------------------------------
cuking_status cuking_roh_samples(cuking_ctx *ctx, const uint64_t *d_bits, uint32_t num_stored,
                                 uint32_t words_per_sample, uint32_t num_sites,
                                 const int32_t *d_group, const uint32_t *d_pos,
                                 uint32_t min_sites, uint32_t min_length, uint32_t bridge_sites,
                                 const uint32_t *d_samples, uint64_t num_samples,
                                 cuking_roh_sample *d_out, cuking_ibd_segment *d_segments,
                                 uint64_t max_segments, uint64_t *num_segments, void *stream) {
  if (num_segments != nullptr) *num_segments = 0;
  // (the arguments first: a refused call touches no device)
  if (ctx == nullptr) return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null context");
  const cuking_status st = cuking_check_roh_args(d_bits, words_per_sample, num_sites, min_sites,
                                                 bridge_sites, num_samples, d_out, d_segments,
                                                 max_segments, num_segments);
  if (st != CUKING_OK) return st;
  if (num_samples == 0) return CUKING_OK;
  return ibd_scan_device(
      ctx, num_sites, d_group, d_pos, max_segments, num_segments, stream,
      [&](const uint64_t *d_group_bits, unsigned long long *d_count, hipStream_t s) {
        return launch_roh_samples(d_bits, num_stored, words_per_sample, num_sites, d_group_bits,
                                  d_pos, min_sites, min_length, bridge_sites, d_samples,
                                  num_samples, d_out, d_segments, max_segments, d_count, s);
      });
}

// ---- Mendelian errors (king_mendel.hip) -----------------------------------------
cuking_status cuking_mendel_trios(cuking_ctx *ctx, const uint64_t *d_bits, uint32_t num_stored,
                                  uint32_t words_per_sample, uint32_t num_sites,
                                  const uint32_t *d_trios, uint64_t num_trios,
                                  cuking_mendel_trio *d_out, uint64_t *d_error_bits,
                                  void *stream) {
  // (the arguments first: a refused call touches no device)
  if (ctx == nullptr) return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null context");
  const cuking_status st =
      cuking_check_mendel_args(d_bits, words_per_sample, num_sites, d_trios, num_trios, d_out);
  if (st != CUKING_OK) return st;
  if (num_trios == 0) return CUKING_OK;
  BIND_OR_RETURN(ctx);
  HIP_TRY(launch_mendel_trios(d_bits, num_stored, words_per_sample, num_sites, d_trios, num_trios,
                              d_out, d_error_bits, (hipStream_t)stream));
  return CUKING_OK;
}

cuking_status cuking_mendel_site_counts(cuking_ctx *ctx, const uint64_t *d_error_bits,
                                        uint64_t num_trios, uint32_t plane_words,
                                        uint32_t *d_counts, void *stream) {
  if (ctx == nullptr) return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null context");
  const cuking_status st =
      cuking_check_mendel_site_args(d_error_bits, num_trios, plane_words, d_counts);
  if (st != CUKING_OK) return st;
  if (num_trios == 0) return CUKING_OK;
  BIND_OR_RETURN(ctx);
  HIP_TRY(launch_mendel_site_counts(d_error_bits, num_trios, plane_words, d_counts,
                                    (hipStream_t)stream));
  return CUKING_OK;
}

// ---- Hardy-Weinberg test (king_hwe.hip) -------------------------------------------
cuking_status cuking_hwe_sites(cuking_ctx *ctx, const uint32_t *d_counts, uint32_t num_sites,
                               uint32_t flags, double *d_p, void *stream) {
  // (the arguments first: a refused call touches no device)
  if (ctx == nullptr) return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null context");
  const cuking_status st = cuking_check_hwe_args(d_counts, num_sites, flags, d_p);
  if (st != CUKING_OK) return st;
  if (num_sites == 0) return CUKING_OK;
  // (the kernel loads a row as one 16-byte word; cuking_site_counts' array is aligned like that)
  if (reinterpret_cast<uintptr_t>(d_counts) % 16 != 0 || reinterpret_cast<uintptr_t>(d_p) % 8 != 0)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                       "hwe sites: d_counts must be 16-byte and d_p 8-byte aligned");
  BIND_OR_RETURN(ctx);
  HIP_TRY(launch_hwe_sites(d_counts, num_sites, (flags & CUKING_HWE_MIDP) != 0, d_p,
                           (hipStream_t)stream));
  return CUKING_OK;
}

cuking_status cuking_ibd_pairs(cuking_ctx *ctx, const uint64_t *d_bits, uint32_t num_stored,
                               uint32_t words_per_sample, uint32_t num_sites,
                               const int32_t *d_group, const uint32_t *d_pos, uint32_t min_sites,
                               uint32_t min_length, const void *d_pairs, uint64_t num_pairs,
                               uint32_t pair_stride, cuking_ibd_pair *d_out,
                               cuking_ibd_segment *d_segments, uint64_t max_segments,
                               uint64_t *num_segments, void *stream) {
  return ibd_pairs_device(ctx, d_bits, num_stored, words_per_sample, num_sites, d_group, d_pos,
                          min_sites, min_length, 0, d_pairs, num_pairs, pair_stride, d_out,
                          nullptr, d_segments, max_segments, num_segments, stream);
}

cuking_status cuking_ibd_pairs_bridged(cuking_ctx *ctx, const uint64_t *d_bits,
                                       uint32_t num_stored, uint32_t words_per_sample,
                                       uint32_t num_sites, const int32_t *d_group,
                                       const uint32_t *d_pos, uint32_t min_sites,
                                       uint32_t min_length, uint32_t bridge_sites,
                                       const void *d_pairs, uint64_t num_pairs,
                                       uint32_t pair_stride, cuking_ibd_pair *d_out,
                                       uint32_t *d_bridged, cuking_ibd_segment *d_segments,
                                       uint64_t max_segments, uint64_t *num_segments,
                                       void *stream) {
  return ibd_pairs_device(ctx, d_bits, num_stored, words_per_sample, num_sites, d_group, d_pos,
                          min_sites, min_length, bridge_sites, d_pairs, num_pairs, pair_stride,
                          d_out, d_bridged, d_segments, max_segments, num_segments, stream);
}

// ---- IBD scan of a block (king_ibd_scan.hip) -----------------------------------
cuking_status cuking_ibd_scan(cuking_ctx *ctx, const uint64_t *d_bits, uint32_t num_stored,
                              uint32_t words_per_sample, uint32_t num_sites,
                              const int32_t *d_group, const uint32_t *d_pos, uint32_t min_sites,
                              uint32_t min_length, const cuking_submatrix *block,
                              uint64_t min_total, cuking_ibd_pair *d_records,
                              uint64_t max_records, uint64_t *num_records, void *stream) {
  if (num_records != nullptr) *num_records = 0;
  // (the arguments first: a refused call touches no device)
  if (ctx == nullptr) return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null context");
  const cuking_status st = cuking_check_ibd_scan_args(d_bits, num_stored, words_per_sample,
                                                      num_sites, min_sites, block, d_records,
                                                      max_records, num_records);
  if (st != CUKING_OK) return st;
  // (without a site no run exists: no record)
  if (sm_num_rows(*block) == 0 || sm_num_cols(*block) == 0 || num_sites == 0) return CUKING_OK;
  return ibd_scan_device(
      ctx, num_sites, d_group, d_pos, max_records, num_records, stream,
      [&](const uint64_t *d_group_bits, unsigned long long *d_count, hipStream_t s) {
        return launch_ibd_scan(d_bits, words_per_sample, num_sites, d_group_bits, d_pos,
                               min_sites, min_length, *block, min_total, d_records, max_records,
                               d_count, s);
      },
      cuking_ibd_scan_count_status);
}

// ---- timing ---------------------------------------------------------------

cuking_status cuking_timing_enable(cuking_ctx *ctx, int enabled) {
  if (ctx == nullptr) return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null context");
  ctx->timing = enabled != 0;
  return CUKING_OK;
}

cuking_status cuking_timing_reset(cuking_ctx *ctx) {
  if (ctx == nullptr) return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null context");
  ctx->king_timer.used = 0;
  ctx->prepare_timer.used = 0;
  return CUKING_OK;
}

cuking_status cuking_timing_collect(cuking_ctx *ctx, double *king_ms,
                                    uint64_t *king_launches, double *prepare_ms,
                                    uint64_t *prepare_launches) {
  BIND_OR_RETURN(ctx);
  double a = 0, b = 0;
  uint64_t na = 0, nb = 0;
  HIP_TRY(ctx->king_timer.collect(&a, &na));
  HIP_TRY(ctx->prepare_timer.collect(&b, &nb));
  if (king_ms) *king_ms = a;
  if (king_launches) *king_launches = na;
  if (prepare_ms) *prepare_ms = b;
  if (prepare_launches) *prepare_launches = nb;
  return CUKING_OK;
}

cuking_status cuking_clock_probe(cuking_ctx *ctx, uint64_t microseconds,
                                 uint64_t *d_ticks, void *stream) {
  BIND_OR_RETURN(ctx);
  if (d_ticks == nullptr) return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null out pointer");
  if (microseconds == 0 || microseconds > 60ull * 1000 * 1000)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "probe time outside (0, 60 s]");
  HIP_TRY(launch_clock_probe(microseconds, d_ticks, (hipStream_t)stream));
  return CUKING_OK;
}

// ---- synthetic inputs -----------------------------------------------------

int cuking_synth_num_models(void) { return kNumSynthModels; }
const char *cuking_synth_model_name(int model) { return synth_model_name(model); }

cuking_status cuking_synth_bitset_model(cuking_ctx *ctx, int model, uint64_t seed,
                                        const uint32_t *d_kind, const uint32_t *d_pa,
                                        const uint32_t *d_pb, uint32_t sample_begin,
                                        uint32_t sample_end, uint32_t num_sites,
                                        uint32_t words_per_sample,
                                        uint64_t *d_bit_set, void *stream) {
  if (model < 0 || model >= kNumSynthModels)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "unknown synthetic cohort model %d", model);
  BIND_OR_RETURN(ctx);
  if (sample_end < sample_begin)
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "sample range reversed");
  if (words_per_sample != cuking_words_per_sample(num_sites))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT,
                "words_per_sample %u does not match %u sites", words_per_sample,
                num_sites);
  if (sample_end > sample_begin && (!d_kind || !d_pa || !d_pb || !d_bit_set))
    return cuking_fail(CUKING_ERR_INVALID_ARGUMENT, "null device pointer");
  if (sample_end == sample_begin || words_per_sample == 0) return CUKING_OK;
  const cuking_status st = grow(ctx, &ctx->synth_tables, &ctx->synth_tables_bytes,
                                synth_table_bytes(sample_end - sample_begin, words_per_sample));
  if (st != CUKING_OK) return st;
  const hipStream_t s = (hipStream_t)stream;
  if (ctx->synth_done == nullptr)
    HIP_TRY(hipEventCreateWithFlags(&ctx->synth_done, hipEventDisableTiming));
  else if (ctx->synth_stream != s)
    HIP_TRY(hipStreamWaitEvent(s, ctx->synth_done, 0));
  HIP_TRY(launch_synth(model, seed, d_kind, d_pa, d_pb, sample_begin, sample_end,
                       num_sites, words_per_sample, ctx->synth_tables, d_bit_set, s));
  HIP_TRY(hipEventRecord(ctx->synth_done, s));
  ctx->synth_stream = s;
  return CUKING_OK;
}

cuking_status cuking_synth_bitset(cuking_ctx *ctx, uint64_t seed,
                                  const uint32_t *d_kind, const uint32_t *d_pa,
                                  const uint32_t *d_pb, uint32_t sample_begin,
                                  uint32_t sample_end, uint32_t num_sites,
                                  uint32_t words_per_sample,
                                  uint64_t *d_bit_set, void *stream) {
  return cuking_synth_bitset_model(ctx, kSynthBaseline, seed, d_kind, d_pa, d_pb, sample_begin,
                                   sample_end, num_sites, words_per_sample, d_bit_set, stream);
}

}  // extern "C"
