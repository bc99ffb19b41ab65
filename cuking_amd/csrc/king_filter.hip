// The filter variant of the KING pair kernel on the gfx950 matrix cores: ONE
// plane product per pair and site instead of four, as a rigorous upper bound on
// kinship, and the exact sums only for the pairs the bound lets through.
//
// With g = -1 / 0 / +1 for hom-ref / het / hom-alt, the reference's numerator
// (cuking.cu:289-294) is -X with
//     X = het_i + het_j - 2 both_het + 4 opposing_hom
//       = sum over the sites defined in both samples of (g_i - g_j)^2
//       = Y_i.D_j + D_i.Y_j - 2 T_i.T_j
// (Y homozygous and defined, D defined, T = R - A; king_mfma.hip "Four
// products").  Y_i.D_j = |Y_i| - Y_i.M_j >= |Y_i| - |M_j| (M missing), and
// het_i = H_i.D_j <= |H_i|, so with the per-sample counts u = |Y| - |M| and |H|
//     X >= u_i + u_j - 2 q,   q = T_i.T_j,
//     kin = 1/2 - X / (4 min(het_i, het_j)) <= 1/2 - (u_i + u_j - 2 q) / (4 min(|H_i|, |H_j|)).
// A pair can only pass `kin > threshold` (0 < threshold < 1/2) when
//     u_i + u_j - 2 q < (2 - 4 threshold) min(|H_i|, |H_j|) + margin,
// the margin (8 sites) covering the float32 roundings of the reference's divide
// and add and of this test (launch_filter's callers keep bitsets below 2^22
// sites, where every term is an exact float).  The slack of the bound is the
// missingness: |M_i| + |M_j| sites, i.e. ~0.01 in kinship at a 1 % missing rate
// with a third of the sites heterozygous; unrelated pairs sit around 0, so at
// the usual thresholds (>= 0.04) next to nothing but real records gets through.
//
// Pipeline per launch chunk (<= kFilterChunkTiles tiles of 256 x 256 pairs):
//   1. king_filter_kernel: q for every pair on the matrix cores (from the
//      two-bit T2 layout, king_common.h: one v_and per fragment dword for either
//      site set; "Offset code" below says what the accumulators carry), the
//      test above per pair; candidates are appended to a list, or, when a 128 x
//      128 quadrant has more than quadrant_cap of them (or the list is full), the
//      quadrant is put on the dense list.  Once most finished quadrants of a
//      launch have gone dense the remaining tiles hand theirs over unexamined.
//   2. king_refine_kernel: one wavefront per candidate, the reference's own six
//      sums straight from the bitset (king_kernels.hip stream kernel), exact
//      kinship, record.  (A relative-counts call, TiledArgs::rel_counts, runs
//      king_refine_count_kernel instead: the four sums kinship needs, its band, two
//      atomics, no record -- and steps 3 and the fallback in their counting form.)
//   3. the four-product kernel (king_mfma.hip, tile-list mode) over the dense
//      quadrants -- nothing, on ordinary cohorts.
// Same records as every other variant, whatever the data: the bound only
// decides WHO computes a pair exactly.
//
// Offset code.  A T2 nibble holds two sites.  Set B (bits 2-3) is T in the fp4
// sign / magnitude code, +-2.0 after `& 0xCCCCCCCC`.  Set A (bits 0-1) is 1 + T in
// plain binary, which `& 0x33333333` leaves as the fp4 values a' = (1 + T) / 2 = 0 /
// 0.5 / 1.0 -- no shift.  A set-A product weighs 1/4, a set-B product 4; the set-B
// MFMAs are the SCALED form of the same instruction with the exact E8M0 scale 2^-2 on
// either operand (byte 0x7D), so that one accumulator holds
//     acc = sum_B T_i T_j / 4 + sum_A a'_i a'_j = (q + n_A + S_i + S_j) / 4,
// S = the sample's sum of T over the set-A sites of the range, n_A their number.  With
// u~ = u + 2 S + n_A per sample (sample_stats_kernel) the value every test needs is
//     u_i + u_j - 2 q = u~_i + u~_j - 8 acc,
// evaluated as (u~_i - 8 acc) + u~_j: acc is a multiple of 1/4 of magnitude <= 2.5
// sites / 4, u~_i - 8 acc = u_i - n_A - 2 S_j - 2 q an integer of magnitude <= 3.5
// sites, the result one of <= 4 sites -- all exact floats up to 2^22 sites
// (kMfmaN4MaxSites), so the value tested is the same float as u_i + u_j - 2 q computed
// from q itself.  u~, S and n_A are sums over sites: prefixes, phase ranges, the wrap of
// a rotated tile and the k-pieces of a split remainder work on differences and sums of
// them like on u -- as long as every partial of such a difference is itself u~ over a
// set of sites (<= 2.5 per site): prefix_u_of() subtracts before it adds the wrapped end.
//
// A workgroup's tile is filter_tile(): take_tile, launch_verdict (tiles that give up leave
// for a gated launch of the four-product kernel), plan_checks ("Check points": a tile none
// of whose pairs can still become a candidate leaves inside the k loop, and so does one that
// holds a few, handing them over; "Rotated tiles": a tile starts where the tiles of its XCD
// are and wraps around, so that they share their operands through the XCD's L2), the k loop
// with check_sweep at its check points, leave_early, reduce_pieces, emit_candidates.  (A
// persistent launch -- one resident workgroup per CU taking tile after tile -- was measured
// 1.2 % slower and removed: r04_tile_gaps.txt.)
//
// Site order (king_sort.hip, TiledArgs::site_curve): the conversion may hand this kernel the
// sites sorted by what they add to X of unrelated pairs.  Nothing in the k loop, the epilogue
// or the refine kernel knows: the sums are over all sites either way.  Only the SHARE in front
// of the rigorous check changes -- taken from the cohort's measured curve (launch_verdict,
// plan_checks) instead of the linear rule -- and where a tile of such a layout rotates: not
// around the end of the sites (that starts a tile on the light sites: measured slower than
// stored order) but inside the head of the order, the sites in front of the check (plan_checks,
// "head lap"; launch_filter says which launches take it).
// configs[2]: 125.2 -> 118.1 ms per step, profiles/r18_site_order.txt; the head lap:
// profiles/r20_head_lap.txt.
//
// Workgroup = 256 x 256 pairs, 4 wavefronts of 128 x 128 = 4 x 4 MFMA blocks (256
// accumulator registers), k-step = 256 sites = 4 slices of 64, 5 LDS stages of
// 32 KiB by LDS-DMA.  Per k-step and wavefront: 64 MFMAs (32 of them scaled), 16
// ds_read_b128, 128 VALU (v_and), 8 requests of 1 KiB.  DESIGN.md 4.0 has the
// measurements; profiles/r03_ablation.txt, r03_filter_curve.txt, r04_l2_probe.txt and
// r04_tile_gaps.txt the raw numbers.
#include <hip/hip_runtime.h>
#include <stdio.h>

#include <atomic>
#include <stdlib.h>

#include "king_common.h"
#include "king_device.h"
#include "king_kin_summary.h"

// The LDS-DMA statements below write M0 and say so in their clobber lists.
#pragma clang diagnostic ignored "-Winline-asm"

namespace cuking {

namespace {

typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));

constexpr int kT = (int)kFilterTile;
// LDS stages: 5 of 32 KiB (two units of 64 sites per k-half: a k-step of 256 sites).
// 10 of 16 KiB (one unit, 8 instead of 3 k-steps of lead) measured the same: configs[2]
// 148.1 -> 148.2 ms (profiles/r03_ablation.txt).
constexpr int kUnits = 2;                             // units per k-half and stage
constexpr int kStages = 5;
constexpr int kSliceU4 = kT;                          // one (side, k-half, unit): 256 samples
constexpr int kStageU4 = 2 * 2 * kUnits * kSliceU4;   // uint4 per stage
constexpr int kStageReqs = 4 * kUnits;                // requests per wavefront and stage
// requests that may be in flight at a hand-over: the stages after next, plus what the
// k-step has issued before its last slice
constexpr int kSyncVm = (kStages - 3) * kStageReqs + (kStageReqs - 2);
static_assert(kSyncVm < 64, "vmcnt is a 6-bit counter");
static_assert(kStages * kStageU4 * 16 == (int)kFilterLdsBytes, "LDS size");
constexpr uint32_t kNoPair = 0xFFFFFFFFu;

// Which stored sample of the reference bitset plane sample `ps` is (the same
// mapping as the prepare kernels), or kNoPair for padding.
__device__ __forceinline__ uint32_t source_sample(const PlaneGeometry &geo, uint32_t ps) {
  if (geo.diag || ps < geo.rows_padded) return ps < geo.num_rows ? ps : kNoPair;
  const uint32_t c = ps - geo.col_base;
  return c < geo.num_cols ? geo.num_rows + c : kNoPair;
}

// One wavefront per plane sample: (u, |H|) = (|Y| - |M|, |H|) as floats (exact below
// 2^24 sites) -- what the sample order is built from.  Padding sites of the last word
// are missing (cuking.cu:513-523) and count as such; padding samples get (0, 0).
// Beside them what the pair test reads ("Offset code" below):
//     u~ = u + 2 S + n_A,   S = the sample's sum of T over the set-A sites (the high
//     32 sites of every 64: the low fields of the T2 layout), n_A = their number
//     (128 per k-step, padding sites included: T = 0 there),
// over all sites (row kNumCum of `cum`) and CUMULATIVE at every phase boundary of the
// k-steps (king_common.h phase_step: cum[x - 1][sample] = over the first 256
// phase_step(x) sites, x = 1 .. 127) -- what a check point of a tile that started at any
// phase needs; u, S and n_A are sums over sites, so differences of u~ serve every range
// --, and the cohort's sums (samples, missing calls, het calls) the kernel picks a check
// from.
struct CheckWords {
  uint32_t w[kNumCheckShares];  // k-steps behind each share from the first site on (0: no checks)
};
constexpr uint32_t kStatsMaxSteps = kMfmaN4MaxSites / 256;  // k-steps of the widest bitset
__global__ __launch_bounds__(256) void sample_stats_kernel(
    const uint64_t *__restrict__ bits, uint32_t words_per_sample, PlaneGeometry geo,
    float2 *__restrict__ stats, float *__restrict__ cum, unsigned long long *__restrict__ sums,
    uint32_t *__restrict__ steps_out, CheckWords cw, uint32_t s_begin, uint32_t s_end) {
  __shared__ uint8_t phase_of[kStatsMaxSteps];  // the phase a k-step belongs to
  __shared__ int32_t phase_sum[4][kNumPhases];  // per wavefront: |Y| - |M| + 2 S per phase
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (blockIdx.x == 0 && threadIdx.x < kNumCheckShares) steps_out[threadIdx.x] = cw.w[threadIdx.x];
  const uint32_t all_steps = geo.k_words / 8;  // k-steps of 256 sites
  // k-step s is in phase x <=> phase_step(x) <= s < phase_step(x + 1)
  //                        <=> x = ceil(64 (s + 1) / all_steps) - 1
  for (uint32_t st = threadIdx.x; st < all_steps; st += 256) {
    const uint32_t x = (kNumPhases * (st + 1) - 1) / all_steps;
    phase_of[st] = (uint8_t)(x < kNumPhases ? x : kNumPhases - 1);
  }
#pragma unroll
  for (uint32_t k = 0; k < kNumPhases / 64; ++k) phase_sum[wave][lane + 64 * k] = 0;
  __syncthreads();
  const uint32_t ps = s_begin + blockIdx.x * 4 + wave;
  if (ps >= s_end) return;  // whole wavefront
  const uint32_t src = source_sample(geo, ps);
  int32_t yc = 0, mc = 0, hc = 0, sa = 0;
  if (src != kNoPair) {
    const uint32_t n = words_per_sample / 2;
    const uint64_t *het = bits + (uint64_t)src * words_per_sample;
    const uint64_t *hom = het + n;
    constexpr uint32_t kAhead = 4;  // words per lane and plane requested before any is counted
    for (uint32_t w0 = 0; w0 < n; w0 += 64 * kAhead) {
      uint64_t h[kAhead], v[kAhead];
#pragma unroll
      for (uint32_t k = 0; k < kAhead; ++k) {
        const uint32_t w = w0 + 64 * k + lane;
        const bool in = w < n;
        h[k] = in ? het[w] : 0ull;
        v[k] = in ? hom[w] : 0ull;
      }
#pragma unroll
      for (uint32_t k = 0; k < kAhead; ++k) {
        const uint32_t w = w0 + 64 * k + lane;
        const bool in = w < n;  // (beyond the plane: contributes nothing)
        const int32_t y = in ? __popcll(~h[k]) : 0;  // homozygous and defined (missing has the het bit set)
        const int32_t m = __popcll(h[k] & v[k]);     // missing
        yc += y;
        mc += m;
        hc += __popcll(h[k] & ~v[k]);  // het
        // (a k-step is 4 words of 64 sites = 4 neighbouring lanes: their sum first, then ONE
        //  LDS add per k-step -- a dozen lanes share a phase)
        // T over the set-A sites of the word: hom-ref minus hom-alt
        const uint64_t hom_a = in ? ~h[k] & 0xFFFFFFFF00000000ull : 0ull;
        const int32_t t_a = __popcll(hom_a & ~v[k]) - __popcll(hom_a & v[k]);
        sa += t_a;
        int32_t d = y - m + 2 * t_a;
        d += __shfl_xor(d, 1);
        d += __shfl_xor(d, 2);
        if ((lane & 3) == 0 && in) atomicAdd(&phase_sum[wave][phase_of[w >> 2]], d);
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      yc += __shfl_xor(yc, off);
      mc += __shfl_xor(mc, off);
      hc += __shfl_xor(hc, off);
      sa += __shfl_xor(sa, off);
    }
  }
  // (the wavefront's own LDS adds are done: same wavefront, in order) inclusive scan over
  // the phases -- lane l holds phases 2 l and 2 l + 1 --: the count in front of boundary x + 1
  // is the scan's value at phase x
  static_assert(kNumPhases == 128, "two phases per lane");
  const int32_t p0 = phase_sum[wave][2 * lane], p1 = phase_sum[wave][2 * lane + 1];
  int32_t run = p0 + p1;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int32_t up = __shfl_up(run, off);
    if ((int)lane >= off) run += up;
  }
  // (n_A in front of boundary x: 128 per k-step)
  cum[(size_t)(2 * lane) * geo.s_stride + ps] =
      (float)(run - p1 + (int32_t)(128u * phase_step(all_steps, 2 * lane + 1)));
  if (2 * lane + 1 < kNumCum)
    cum[(size_t)(2 * lane + 1) * geo.s_stride + ps] =
        (float)(run + (int32_t)(128u * phase_step(all_steps, 2 * lane + 2)));
  if (lane == 0) {
    stats[ps] = make_float2((float)(yc - mc), (float)hc);
    cum[(size_t)kNumCum * geo.s_stride + ps] = (float)(yc - mc + 2 * sa + (int32_t)(128u * all_steps));
    // (the cohort's sums feed a choice, not a result: a sample of the samples will do --
    //  three device-scope atomics on three addresses for EVERY sample cost 3 ms at 100k)
    if (src != kNoPair && ((blockIdx.x & 15) == 0 || gridDim.x < 64)) {
      relaxed_add(sums, 1ull);
      relaxed_add(sums + 1, (unsigned long long)mc);
      relaxed_add(sums + 2, (unsigned long long)hc);
    }
  }
}

__device__ __forceinline__ v16f mma(const v8i a, const v8i b, const v16f c) {
  // scale operands 0: the unscaled instruction
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 4 /* fp4 */, 4, 0, 0, 0, 0);
}

// The scaled form: both operands times the E8M0 scale in byte 0 of `scale` (a VGPR).
__device__ __forceinline__ v16f mma_scaled(const v8i a, const v8i b, const v16f c, const int scale) {
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 4 /* fp4 */, 4, 0, scale, 0, scale);
}

__device__ __forceinline__ v8i tfrag(const uint4 w, uint32_t mask) {
  v8i r = {0, 0, 0, 0, 0, 0, 0, 0};
  r[0] = (int)(w.x & mask);
  r[1] = (int)(w.y & mask);
  r[2] = (int)(w.z & mask);
  r[3] = (int)(w.w & mask);
  return r;
}

// ---- The phases of a tile, in the order filter_tile() (at the end) calls them: all inlined into
// the one kernel; each sees of the others what its parameters and its result say.
// The tile (or the piece of the k range of one) a workgroup has taken.  Wave-uniform.
struct Tile {
  bool split;            // a piece of one of the launch's last tiles (king_common.h, fsplit_*)
  uint32_t bid;          // the tile's index within the launch
  uint32_t tr, tc;       // its row and column in the tile space
  uint32_t part, piece;  // split: the part of the k range, the piece's index within the launch
};

// The level of the bound for the cohort's unrelated pairs: its mean m (1 + m / (2 h (1 - m)))
// at the cohort's missing rate m and het rate h (from its sums: samples, missing calls, het
// calls) and its standard deviation 1 / sqrt(sites) (tools/bound_tiers.py,
// profiles/r04_bound_tiers.txt).  False for a cohort without samples or het calls.
__device__ __forceinline__ bool bound_level(const unsigned long long *cohort_sums, float sites,
                                            float *mean, float *sigma) {
  const float ns = (float)cohort_sums[0], nm = (float)cohort_sums[1], nh = (float)cohort_sums[2];
  if (!(ns > 0.f && nh > 0.f)) return false;
  const float m = nm / (ns * sites), h = nh / (ns * sites);
  *mean = m * (1.f + m / (2.f * h * (1.f - m)));
  *sigma = rsqrtf(sites);
  return true;
}

// Which tile workgroup `wg` of a grid of one workgroup per tile takes.  False (uniform, before
// anything else) when there is none: the dynamic tail is through, or the workgroup is padding.
__device__ __forceinline__ bool take_tile(const TiledArgs &a, const uint32_t wg, uint4 *const lds,
                                          Tile *t) {
  uint32_t bid = wg;
  // Remainder of a short launch (king_common.h, fsplit_*): piece `part` of the k
  // range of one of the launch's last tiles.
  t->split = a.fsplit_parts != 0 && wg >= a.fsplit_first;
  t->part = t->piece = 0;
  if (t->split) {
    t->piece = wg - a.fsplit_first;
    t->part = __builtin_amdgcn_readfirstlane(t->piece % a.fsplit_parts);
    bid = a.fsplit_tile0 + t->piece / a.fsplit_parts;
  } else
  if (a.dyn_tiles != 0 && wg >= a.launch_tiles) {
    // dynamic tail (king_common.h): the next of the launch's last dyn_tiles tiles
    // nobody has taken yet -- the XCDs run at rates a few percent apart, and an
    // XCD that gets through its static share early takes more of these.  (The
    // counter is filter_ctrl[2], zeroed in front of every launch.)
    uint32_t *slot = reinterpret_cast<uint32_t *>(lds);
    if (threadIdx.x == 0) *slot = relaxed_add(a.filter_ctrl + kCtrlDyn, 1u);
    __syncthreads();
    const uint32_t next = __builtin_amdgcn_readfirstlane(*slot);
    __syncthreads();  // the word is stage memory from here on
    if (next >= a.dyn_tiles) return false;  // uniform: nothing left
    bid = a.launch_tiles + next;
  } else if (a.xcd_chunk == 1) {
    // patches of 32 consecutive tiles dealt round-robin to the XCDs (king_common.h)
    bid = xcd_patch_tile(bid);
    if (bid >= a.launch_tiles) return false;  // padding (uniform)
  }
  t->bid = __builtin_amdgcn_readfirstlane(bid);
  uint32_t tr, tc;
  if (!decode_tile_space(a, a.tile_begin + t->bid, &tr, &tc)) return false;  // uniform
  t->tr = __builtin_amdgcn_readfirstlane(tr);
  t->tc = __builtin_amdgcn_readfirstlane(tc);
  return true;
}

// The launch-wide verdict, for a whole tile of a launch with a fallback (a.tile_done): true
// when the tile gives up.
// When the bound does not thin this cohort out (a threshold inside the noise of
// unrelated pairs, heavy missingness) nearly every quadrant ends on the dense list
// anyway: once most of at least 512 finished quadrants of the launch have (or their
// tiles have left at check 0, below), every remaining tile leaves at once -- it
// touches nothing, and the fallback launch behind this one (the four-product kernel
// over the chunk in its own order, king_mfma.hip persistent mode) computes every tile
// that has not set its tile_done flag.  The worst case costs the exact kernel's time
// plus the first round of this one (short launches: plus an eighth of it, check 0).
// *xcd_pos: the k-step the tiles of this XCD are at (rotated tiles, plan_checks()).
// *order_share: site order only (TiledArgs::site_curve) -- the share of the sites from the
// first on that stands in front of the rigorous check, in 64ths: the HEAD of the order
// (0 = the curve allows none up to 62/64).  The same for every tile of the launch.
__device__ __forceinline__ bool launch_verdict(const TiledArgs &a, const uint32_t wg,
                                               uint4 *const lds, uint32_t *xcd_pos,
                                               uint32_t *order_share) {
  // ONE decision per workgroup (the counters move while the wavefronts read them,
  // and a wavefront that left alone would take its quarter of every stage's
  // requests with it): thread 0 reads, the stage memory carries the verdict.
  uint32_t *verdict = reinterpret_cast<uint32_t *>(lds);
  if (threadIdx.x == 0) {
    uint32_t leave = relaxed_load(a.filter_ctrl + kCtrlAllLeave);
    // (the first to find out says so: to the tiles behind it, and to the fallback launch)
    auto all_leave = [&] {
      leave = 1;
      relaxed_store(a.filter_ctrl + kCtrlAllLeave, 1u);
      relaxed_store(a.filter_ctrl + kCtrlGate, 1u);
    };
    // The cohort's own verdict first: where the bound's level for unrelated pairs (from the
    // cohort's mean missing and het rates, as for the check points below) lies four
    // standard deviations above the threshold, it lets every pair through, whatever the
    // tile -- the first tiles need not find that out by computing their product.
    float mean, sigma;
    if (leave == 0 && a.cohort_sums != nullptr && a.check_steps != nullptr &&
        bound_level(a.cohort_sums, 32.f * (float)a.geo.k_words, &mean, &sigma) &&
        mean - 4.f * sigma > a.kin_threshold && (a.check1 >> 16) != 0)
      all_leave();
    if (leave == 0) {
      const uint32_t dense_so_far =
          relaxed_load(a.filter_ctrl + kCtrlDense) + relaxed_load(a.filter_ctrl + kCtrlLeft);
      const uint32_t finished = relaxed_load(a.filter_ctrl + kCtrlFinished);
      if (finished >= 512 && 2 * dense_so_far > finished) all_leave();
    }
    verdict[0] = leave;
  }
  // Rotated tiles (below): where the tiles of this XCD are -- workgroups go to the XCDs
  // round-robin by their index.  Every slot says where one of them was and when; brought
  // forward to now by the measured k-step time, the most advanced one counts.
  if (a.rotate == 1 && threadIdx.x < kPosSlots) {
    const uint32_t x = wg & 7;
    const unsigned long long said = relaxed_load(
        reinterpret_cast<const unsigned long long *>(a.filter_ctrl + kCtrlPos) + x * kPosSlots +
        threadIdx.x);
    const uint32_t ticks16 = relaxed_load(a.filter_ctrl + kCtrlStepTicks + x);
    uint32_t pos = (uint32_t)(said >> 32);
    const uint32_t ago = (uint32_t)__builtin_amdgcn_s_memrealtime() - (uint32_t)said;
    if (said != 0 && ticks16 != 0 && ago < 16384u)
      pos += ago * 16u / ticks16;
    verdict[1 + threadIdx.x] = pos;
  }
  // Site order: X does not grow linearly in the site index, the conversion has left the
  // curve (king_common.h SiteCurve).  The share becomes the first 64th (32 .. 62) behind
  // which the tile has seen `need` of an unrelated pair's X: need = (1 - 2 thr) / (1 - 2
  // kappa) as in stored order ("Check points" below), kappa with the standard deviation the
  // site counts give.  One wavefront tries every share at once, one word carries the
  // answer to the workgroup (ONE decision per workgroup, as above).  It need not be thread
  // 0's wavefront: unlike the counters above, the curve and the cohort's sums are written by
  // the conversion in front of the launch and do not change while it runs, so every reader
  // sees one snapshot; the stage memory still carries the one answer.
  if (a.site_curve != nullptr && (threadIdx.x >> 6) == 1) {
    const uint32_t s = threadIdx.x & 63;
    float mean, sigma;
    bool ok = false;
    if (a.cohort_sums != nullptr &&
        bound_level(a.cohort_sums, 32.f * (float)a.geo.k_words, &mean, &sigma)) {
      const float kappa = mean + 4.6f * a.site_curve->sigma + 0.003f;
      const float need = (1.f - 2.f * a.kin_threshold) / (1.f - 2.f * kappa);
      ok = kappa < 0.5f && s >= 32 && s <= 62 &&
           site_curve_covers(a.site_curve->cum, 0, s, need);
    }
    const unsigned long long fits = __ballot(ok);
    if (s == 0) verdict[1 + kPosSlots] = fits != 0 ? (uint32_t)__ffsll(fits) - 1u : 0u;
  }
  __syncthreads();
  *order_share = a.site_curve != nullptr ? __builtin_amdgcn_readfirstlane(verdict[1 + kPosSlots]) : 0u;
  const bool give_up = verdict[0] != 0;
  uint32_t pos = 0;
  if (a.rotate == 1) {
#pragma unroll
    for (uint32_t k = 0; k < kPosSlots; ++k) pos = max(pos, verdict[1 + k]);
  }
  *xcd_pos = __builtin_amdgcn_readfirstlane(pos);
  __syncthreads();  // the words are stage memory from here on
  // uniform across the workgroup; tile_done stays 0
  // (its quadrants count as handed over: "filter_dense_quadrants")
  if (give_up && threadIdx.x == 0) relaxed_add(a.filter_totals + kTotalDense, 4ull);
  return give_up;
}

// --- Check points (king_common.h).  X = sum over the sites of (g_i - g_j)^2 has only
// non-negative terms, so its sum over a PREFIX of the sites is a lower bound of X, and
// so is this kernel's bound of that prefix sum, u'_i + u'_j - 2 q' (u' over the prefix,
// sample_stats_kernel).  A pair can only pass the threshold when X < t min(|H_i|, |H_j|) +
// margin (|H| over ALL sites: the epilogue's own test): a tile none of whose 65,536 pairs
// satisfies u'_i + u'_j - 2 q' < that bound at the check point holds no record, whatever
// the remaining sites say -- it leaves.  For unrelated samples that happens from a share
// (1 - 2 thr) / (1 - 2 kappa) of the sites on, kappa = the level of the bound for unrelated
// pairs (bound_level() above: its mean plus 4.6 standard deviations): 0.88 of the sites at
// the default threshold and 1 % missing calls.  Every workgroup picks
// the same entry of the share menu from the cohort's sums.  (Check 0 is a FORECAST for
// short launches: the same test with the bound scaled to an eighth of the sites, counted
// per quadrant; a tile whose quadrants mostly look dense leaves for the exact kernel
// there instead of at its end.)  The pipeline is DRAINED at a check point -- the segment
// before it ends like a tile (every request landed, no fragment built ahead), the one
// behind it starts like a tile -- so that the check has the LDS for its per-sample
// values and the register file for its sweep, and the k loop's registers are not live
// across it: ~8 us per check of a 500 us tile.
//
// --- Rotated tiles.  The 32 tiles an XCD holds at a time are a patch of the tile space
// (8 rows x 4 columns: 12 strips of operands for 32 tiles), but they share those strips
// through the XCD's 4 MiB L2 only while they read the same k-steps at about the same
// time -- 21 k-steps of the patch fit.  Tiles that all start at k-step 0 do so in the
// first round of a launch and drift apart from there (L2 hit rate 0.36, 555 GB from the
// fabric per pass of configs[2]; one launch per round: 0.80 and 170 GB, and the chip
// holds 1.96-1.99 GHz instead of 1.86: tools/l2_probe.sh).  The order of the sites
// inside a sum does not matter, so a tile STARTS where the tiles of its XCD are: at the
// phase boundary (king_common.h phase_step: 128 phases) nearest to the k-step the most
// advanced of them has published, runs to the end of the sites, wraps around (a segment
// boundary like a check point's) and ends where it started.  A check point sits behind a
// share of the k-steps as before; the per-sample counts over "phases [p, p + e)" are
// differences of the cumulative counts sample_stats_kernel leaves.
struct CheckPlan {
  uint32_t chk0, chk1;  // k-steps of the tile in front of check 0 / check 1 (0: no such check)
  uint32_t share1;      // the share of the sites in front of check 1, in 64ths
  uint32_t phase;       // the phase boundary the tile starts at (0: not rotated)
  uint32_t k0;          // ... as a k-step of the bitset
  uint32_t wrap;        // k-steps of the tile in front of the end of its ring (0: none behind)
  uint32_t ring;        // the k-steps the tile goes around: all of them, or the head's (lap)
  uint32_t count_phase; // the phase boundary the counts at a check start at: `phase`, lap: 0
  uint32_t start_abs;   // k0, counted on from the position the XCD's tiles have published
};
// `xcd_pos`, `order_share`: launch_verdict(); `all_steps`: the bitset's k-steps, `num_steps`:
// the tile's.
// --- Site order (TiledArgs::site_curve; king_sort.hip).  The prefix bound does not care WHICH
// sites the prefix holds, so the conversion may put the sites that contribute most to X of
// unrelated pairs in front; the share H (64ths) then comes from the cohort's measured curve
// (launch_verdict) instead of the linear rule.  A tile that wrapped around the END of the
// sites would begin with the light ones, so a tile of such a layout rotates inside the HEAD
// of the order instead -- the head lap: it starts at a phase p in [0, 2 H), runs to the end
// of the head (k-step kH), wraps to the first site and runs up to p.  There it has summed
// exactly the head's sites, in another order: the rigorous check is the unrotated tile's,
// on the same counts (those in front of boundary 2 H, nothing subtracted), and only a tile
// that stays goes on into the tail [kH, all_steps).  The ring the XCD's tiles share is the
// head's kH k-steps: positions are published and joined modulo kH, and a tile in its tail
// says nothing.  Without a lap (no share, a forced menu entry, a forecast check in this
// launch, a head shorter than rotate_min_steps) such a tile is not rotated.
__device__ __forceinline__ CheckPlan plan_checks(const TiledArgs &a, const Tile &t,
                                                 const uint32_t xcd_pos, const uint32_t order_share,
                                                 const uint32_t all_steps,
                                                 const uint32_t num_steps) {
  uint32_t chk0 = 0, chk1 = 0, entry1 = 0, share1 = 0;
  uint32_t phase = 0, k0 = 0, wrap = 0, start_abs = 0, ring = all_steps;
  bool lap = false;
  if (!t.split && a.check_steps != nullptr && a.tile_done != nullptr) {
    // kappa: the level of the bound for this cohort's unrelated pairs (from its mean missing
    // and het rates) plus 4.6 standard deviations and a little
    float kappa = -1.f, mean, sigma;
    if (bound_level(a.cohort_sums, 256.f * (float)all_steps, &mean, &sigma))
      kappa = mean + 4.6f * sigma + 0.003f;
    // Check 0 (the forecast; a.check0: 1 = this is a short launch, 2 = forced): only for a
    // cohort whose unrelated pairs come anywhere near the threshold -- a drain and a sweep
    // per tile (1.5-3 % of configs[1]) that a clean cohort need not pay; a cohort that is
    // clean on average but holds a few bad samples then carries its dense tiles to their
    // end before the quadrant lists take them over.  (The same for every tile of a launch.)
    const bool take0 = (a.check0 == 2 || (a.check0 == 1 && kappa > 0.7f * a.kin_threshold)) &&
                       a.check_steps[0] != 0;
    const uint32_t sw1 = a.check1 & 0xFFu;
    // the ring: every k-step (stored order), or the head's (site order, the head lap)
    const uint32_t head = order_share * kPhasesPerShare;  // phases
    const uint32_t k_head = phase_step(all_steps, head);
    lap = a.site_curve != nullptr && a.rotate != 0 && order_share != 0 && sw1 == 1 && !take0 &&
          a.check_steps[1] != 0 && k_head >= a.rotate_min_steps && k_head < num_steps;
    if (lap) ring = k_head;
    const uint32_t ring_phases = lap ? head : kNumPhases;
    if (a.rotate != 0 && (lap || (a.site_curve == nullptr && all_steps >= a.rotate_min_steps))) {
      uint32_t base = 0;
      if (a.rotate == 1) {
        const uint32_t r = xcd_pos % ring;
        base = xcd_pos - r;
        phase = (r * kNumPhases + all_steps / 2) / all_steps;  // (the boundary nearest to r)
      } else if (a.rotate == 2) {
        phase = ((t.bid * 37u + 11u) & (kNumPhases - 1)) % ring_phases;  // (test hook)
      } else {
        phase = ((a.rotate - 3u) & (kNumPhases - 1)) % ring_phases;    // (test hook)
      }
      k0 = phase_step(all_steps, phase);
      // (the ring's end is its beginning, one turn on -- also where a short bitset puts a
      //  boundary inside the ring on the ring's last k-step)
      if (phase >= ring_phases || k0 >= ring) {
        phase = 0;
        k0 = 0;
        base += ring;
      }
      start_abs = base + k0;
      wrap = k0 != 0 ? ring - k0 : 0u;
    }
    // k-steps from phase boundary `phase` on that cover `share` phases (around the end;
    // stored order, or an unrotated tile: a lap's one check sits behind the ring)
    auto steps_of = [&](uint32_t share) {
      const uint32_t hi = phase + share * kPhasesPerShare;
      return hi <= kNumPhases ? phase_step(all_steps, hi) - k0
                              : (all_steps - k0) + phase_step(all_steps, hi - kNumPhases);
    };
    if (take0) chk0 = steps_of(kCheckShares64[0]);
    if (sw1 >= 2) {
      entry1 = sw1 - 2;
    } else if (sw1 == 1 && a.site_curve != nullptr) {
      // (site order: the share the curve gives, the head)
      if (order_share != 0) {
        share1 = order_share;
        entry1 = 1;
      }
    } else if (sw1 == 1 && kappa >= 0.f) {
      // The share behind which no unrelated pair of this cohort is still under the bound, in
      // 64ths, rounded up -- any of them: the counts are there at every phase boundary.  (A
      // check costs a tile that leaves ~1.5 % -- the drain, the sweep -- and one that stays
      // ~3 % -- the refill as well; a tile that still holds a few live pairs leaves all the
      // same, handing them over, so the share needs no margin: up to 62/64.  The menu of
      // king_common.h is what "filter_check1" = 2 + k forces.)
      const float f64 = 64.f * (1.f - 2.f * a.kin_threshold) / (1.f - 2.f * kappa);
      if (f64 <= 62.f) {
        share1 = (uint32_t)ceilf(f64);
        if (share1 < 32) share1 = 32;
        entry1 = 1;  // (any entry of the menu: whether the bitset is long enough for checks)
      }
    }
#pragma unroll
    for (uint32_t k = 1; k < kNumCheckShares; ++k)
      if (sw1 >= 2 && k == entry1) share1 = kCheckShares64[k];
    // (a lap: behind one turn of the ring, wherever the tile started)
    if (share1 != 0 && a.check_steps[entry1] != 0) chk1 = lap ? ring : steps_of(share1);
    if (chk0 >= num_steps) chk0 = 0;
    if (chk1 >= num_steps || chk1 <= chk0) chk1 = 0;
  }
  auto sgpr = [](uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane(v); };
  return CheckPlan{sgpr(chk0), sgpr(chk1), sgpr(share1), sgpr(phase), sgpr(k0),
                   sgpr(wrap), sgpr(ring), sgpr(lap ? 0u : phase), sgpr(start_abs)};
}

// u~ of plane sample idx over the `share` phases from the tile's first on (`total`: over
// all sites): cumulative counts in front of the inner boundaries, nothing in front of 0.
// A range that goes around the end of the sites is (total - front of `phase`) + front of
// the wrapped end, in THAT order: every partial is then u~ over a contiguous range of
// sites or over two disjoint ones, at most 2.5 per site -- total + the wrapped end first
// would reach 5 per site, past 2^24 at 2^22 sites (king_common.h, kMfmaN4MaxSites).
// (A head lap has covered the head from the first site on, whatever its phase: count_phase 0.)
__device__ __forceinline__ float prefix_u_of(const TiledArgs &a, const CheckPlan &p,
                                             uint32_t share, size_t idx, float total) {
  const uint32_t s_stride = a.geo.s_stride;
  const uint32_t from = p.count_phase;
  const uint32_t hi = from + share * kPhasesPerShare;  // (uniform; hi < 2 kNumPhases)
  float u = hi >= kNumPhases ? total
            : hi != 0        ? a.prefix_u[(size_t)(hi - 1) * s_stride + idx]
                             : 0.f;
  if (from != 0) u -= a.prefix_u[(size_t)(from - 1) * s_stride + idx];
  if (hi > kNumPhases) u += a.prefix_u[(size_t)(hi - kNumPhases - 1) * s_stride + idx];
  return u;
}

// What a sweep over the tile's pairs reads per sample, staged in the (idle) stage memory by
// the workgroup's 256 threads: (u~, scale (t |H| + margin)) of the tile's 256 row and 256
// column samples, t = 2 - 4 thr; u~ over all sites, or (`prefix`, uniform) over the `share`
// phases from the tile's first on.  Returns the rows' 256 values, the columns' are behind
// them; barrier behind the stores.
__device__ __forceinline__ const float2 *stage_bounds(const TiledArgs &a, const Tile &t,
                                                      const CheckPlan &p, uint4 *const lds,
                                                      const bool prefix, const uint32_t share,
                                                      const float thr, const float scale) {
  float2 *const rows = reinterpret_cast<float2 *>(lds), *const cols = rows + kT;
  const float tt = 2.f - 4.f * thr;
  const size_t ir = (size_t)t.tr * kT + threadIdx.x;
  const size_t ic = (size_t)a.geo.col_base + (size_t)t.tc * kT + threadIdx.x;
  float2 r = a.sample_stats[ir], c = a.sample_stats[ic];
  if (prefix) {
    r.x = prefix_u_of(a, p, share, ir, r.x);
    c.x = prefix_u_of(a, p, share, ic, c.x);
  }
  r.y = scale * fmaf(tt, r.y, 8.f);
  c.y = scale * fmaf(tt, c.y, 8.f);
  rows[threadIdx.x] = r;
  cols[threadIdx.x] = c;
  __syncthreads();
  return rows;
}

// How a tile came out of its k loop (uniform): it ran to its end, or it left at a check
// point: at the forecast, or at the rigorous check -- with nothing alive, or with a few live
// pairs that the epilogue (run on the prefix counts) hands to the candidate list.
enum Leave : uint32_t { kStays = 0, kLeftForecast, kLeftEmpty, kLeftEmit };

// The test at a check point (the pipeline is drained, the stage memory idle): the forecast
// (check 0), or the rigorous check behind share1 of the tile's sites.
__device__ __forceinline__ Leave check_sweep(const TiledArgs &a, const Tile &t, const CheckPlan &p,
                                             const v16f (&acc)[4][4], uint4 *const lds,
                                             const bool forecast, const uint32_t all_steps) {
  const Lanes l = lanes_of_thread();
  // (site order: the forecast's prefix holds that share of an unrelated pair's X, not an eighth)
  const float scale = !forecast ? 1.f
                      : a.site_curve != nullptr
                          ? site_curve_mass(a.site_curve->cum, p.count_phase, kCheckShares64[0])
                          : (float)kCheckShares64[0] * (1.f / 64.f);
  const uint32_t share = forecast ? kCheckShares64[0] : p.share1;  // (uniform)
  // (the forecast counts the pairs that WILL be candidates from an eighth of the sites:
  //  the bound of an unrelated pair scatters sqrt(8) times as widely there as at the
  //  end, 1 / sqrt(sites).  A quadrant goes dense from 2.3 % candidates on -- pairs two
  //  standard deviations out --, so the prefix count matches the final one at that
  //  point when the prefix is tested against a threshold 2 (sqrt(8) - 1) standard
  //  deviations higher; tested against the threshold itself it called cohorts dense that
  //  the list handles at a third of the cost: 7 % missing calls at the default threshold,
  //  profiles/r04_missing_curve.txt)
  const float thr_f = forecast ? a.kin_threshold + 3.66f * rsqrtf(256.f * (float)all_steps)
                               : a.kin_threshold;
  // (u~ over the prefix, scaled bound)
  const float2 *const ck_rows = stage_bounds(a, t, p, lds, true, share, thr_f, scale);
  const float2 *const ck_cols = ck_rows + kT;
  uint32_t *const ck_words = reinterpret_cast<uint32_t *>(lds) + 4 * kT;  // behind them: one per wavefront
  const uint32_t emit_cap = (a.check1 >> 8) & 0xFFu;  // (uniform; king_common.h check1)
  uint32_t cnt = 0;  // pairs of this lane still under the bound
  {
    float2 cc[4];
#pragma unroll
    for (int bj = 0; bj < 4; ++bj) cc[bj] = ck_cols[l.wx * 128 + bj * 32 + l.lr];
#pragma unroll
    for (int bi = 0; bi < 4; ++bi)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float2 cr = ck_rows[l.wy * 128 + bi * 32 + c_row(r, l.g)];
        // (every element of the tile counts, the ones outside the block too: a tile on the
        //  diagonal holds each sample against itself and stays -- 0.5 % of the tiles at
        //  configs[2]; the test on the indices made the kernel a quarter longer)
#pragma unroll
        for (int bj = 0; bj < 4; ++bj)
          cnt += fmaf(-8.f, acc[bi][bj][r], cr.x) + cc[bj].x < fminf(cr.y, cc[bj].y) ? 1u : 0u;
      }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
  // (forecast: twice the cap -- the pairs of a quadrant share their samples, so the count
  //  of a quadrant scatters more widely than independent pairs would; at 7 % missing calls
  //  and the default threshold a sixth of the tiles left with the cap itself, for a launch
  //  the candidate list handles in half the time)
  // (rigorous check: the word carries the quadrant's live pairs, capped -- a tile with
  //  only a FEW of them, the relatives it holds, hands exactly those to the candidate list
  //  and leaves as well: a cohort with some relatedness in every tile keeps its early exits)
  if (l.lane == 0)
    ck_words[l.wave] = forecast ? (cnt > 2 * a.quadrant_cap ? 1u : 0u)
                                : (cnt > emit_cap ? emit_cap + 1 : cnt);
  __syncthreads();
  uint32_t found = forecast ? ck_words[0] + ck_words[1] + ck_words[2] + ck_words[3]
                            : max(max(ck_words[0], ck_words[1]), max(ck_words[2], ck_words[3]));
  found = __builtin_amdgcn_readfirstlane(found);
  __syncthreads();  // (the words are stage memory again from here on)
  if (forecast) return found >= 3 ? kLeftForecast : kStays;
  return found > emit_cap ? kStays : found != 0 ? kLeftEmit : kLeftEmpty;
}

// The book-keeping behind the k loop.  True when the tile left at a check point with
// nothing to hand over: the workgroup is through.
__device__ __forceinline__ bool leave_early(const TiledArgs &a, const Tile &t, const CheckPlan &p,
                                            const Leave left) {
  if (left == kLeftEmit && threadIdx.x == 0) relaxed_add(a.filter_totals + kTotalEarly, 1ull);
  if (p.phase != 0 && threadIdx.x == 0) relaxed_add(a.filter_totals + kTotalRotated, 1ull);
  if (left == kLeftForecast || left == kLeftEmpty) {
    // Forecast: the tile leaves for the exact kernel -- its quadrants count as handed
    // over, the fallback launch is needed.  Rigorous check: for good.
    if (threadIdx.x == 0) {
      relaxed_add(a.filter_ctrl + kCtrlFinished, 4u);
      if (left == kLeftForecast) {
        relaxed_add(a.filter_ctrl + kCtrlLeft, 4u);
        relaxed_store(a.filter_ctrl + kCtrlGate, 1u);
        relaxed_add(a.filter_totals + kTotalDense, 4ull);
      } else {
        a.tile_done[t.bid] = 1;
        relaxed_add(a.filter_totals + kTotalEarly, 1ull);
      }
    }
    return true;
  }
  // This tile runs to its end here: the fallback launch has nothing to do for it.
  // (The tiles of remainder pieces are marked by the host.)
  if (!t.split && a.tile_done != nullptr && threadIdx.x == 0) a.tile_done[t.bid] = 1;
  return false;
}

// A piece of a split tile: park this piece (16-byte write-through stores, [4 registers]
// [thread]), take a ticket of the tile; the last piece in adds the others to its own and
// carries on (true) -- the others are through.
__device__ __forceinline__ bool reduce_pieces(const TiledArgs &a, const Tile &t, v16f (&acc)[4][4],
                                              uint4 *const lds) {
  typedef uint32_t v4u __attribute__((ext_vector_type(4)));
  constexpr uint32_t kSlabU4 = 64 * 256;  // float4 per slab
  {
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        a.fsplit_slabs + (size_t)t.piece * kSlabU4, 0, (int)(kSlabU4 * 16), 0x00020000);
#pragma unroll
    for (int bi = 0; bi < 4; ++bi)
#pragma unroll
      for (int bj = 0; bj < 4; ++bj)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          const v16f &c = acc[bi][bj];
          const v4u v = {__float_as_uint(c[4 * r4]), __float_as_uint(c[4 * r4 + 1]),
                         __float_as_uint(c[4 * r4 + 2]), __float_as_uint(c[4 * r4 + 3])};
          __builtin_amdgcn_raw_buffer_store_b128(
              v, rsrc, (int)((((bi * 4 + bj) * 4 + r4) * 256 + threadIdx.x) * 16), 0,
              16 /* sc1 */);
        }
  }
  // every wavefront's stores are done (and written through), then the ticket
  // (cdna_hip_programming.md, Guideline 16: sc1 payload + counter)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  uint32_t *flag = reinterpret_cast<uint32_t *>(lds);  // the stages are idle now
  if (threadIdx.x == 0) {
    uint32_t *counter = a.fsplit_tickets + t.piece / a.fsplit_parts;
    const uint32_t ticket = relaxed_add(counter, 1u);
    const bool last = ticket == a.fsplit_parts - 1;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      *counter = 0;  // ready for the next launch
    }
    *flag = last ? 1u : 0u;
  }
  __syncthreads();
  const bool last = *flag != 0;
  __syncthreads();  // (the flag word becomes the epilogue's scratch)
  if (!last) return false;
  const uint32_t first_piece = t.piece - t.part;
  for (uint32_t p = 0; p < a.fsplit_parts; ++p) {
    if (p == t.part) continue;
    const float4 *src = a.fsplit_slabs + (size_t)(first_piece + p) * kSlabU4 + threadIdx.x;
#pragma unroll
    for (int bi = 0; bi < 4; ++bi)
#pragma unroll
      for (int bj = 0; bj < 4; ++bj)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          const float4 v = src[((bi * 4 + bj) * 4 + r4) * 256];
          acc[bi][bj][4 * r4] += v.x;
          acc[bi][bj][4 * r4 + 1] += v.y;
          acc[bi][bj][4 * r4 + 2] += v.z;
          acc[bi][bj][4 * r4 + 3] += v.w;
        }
  }
  return true;
}

// The epilogue: the bound, per pair; the candidates go to the list, or their quadrant to the
// dense list.  `on_prefix`: the tile left at the rigorous check with a few live pairs: the
// same test on the sums and the per-sample counts of the sites so far -- every record is
// among the pairs it admits ("Check points" above).  Wavefronts return one by one.
__device__ __forceinline__ void emit_candidates(const TiledArgs &a, const Tile &t,
                                                const CheckPlan &p, const v16f (&acc)[4][4],
                                                uint4 *const lds, const bool on_prefix) {
  const Lanes l = lanes_of_thread();
  // (u~, t |H| + margin) per row and per column
  const float2 *const st_rows = stage_bounds(a, t, p, lds, on_prefix, p.share1, a.kin_threshold, 1.f);
  const float2 *const st_cols = st_rows + kT;
  float2 sc[4];
#pragma unroll
  for (int bj = 0; bj < 4; ++bj) sc[bj] = st_cols[l.wx * 128 + bj * 32 + l.lr];

  // Nearly every wavefront has no candidate at all: a first sweep with the bare test
  // (5 VALU per pair, the largest `bound - x_lb` of the lane: positive <=> the test
  // below holds for some pair, the sign of a float difference is exact; pairs outside
  // the block may raise a false alarm, which only costs the sweeps below), then out.
  {
    float best = -1.f;
#pragma unroll
    for (int bi = 0; bi < 4; ++bi)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float2 sr = st_rows[l.wy * 128 + bi * 32 + c_row(r, l.g)];
#pragma unroll
        for (int bj = 0; bj < 4; ++bj)
          best = fmaxf(best, fminf(sr.y, sc[bj].y) -
                                 (fmaf(-8.f, acc[bi][bj][r], sr.x) + sc[bj].x));
      }
    if (l.lane == 0) relaxed_add(a.filter_ctrl + kCtrlFinished, 1u);
    if (__ballot(best > 0.f) == 0) return;  // wave-uniform
  }

  uint32_t total = 0, base = 0, run = 0;  // wave-uniform
#pragma nounroll
  for (int pass = 0; pass < 2; ++pass) {  // 0: count the candidates, 1: append them
    // (opaque per pass: otherwise the compiler computes the 256 pairs' indices and
    //  validity once in front of the loop and parks them in scratch memory)
    uint32_t tr_p = t.tr, tc_p = t.tc;
    asm volatile("" : "+s"(tr_p), "+s"(tc_p));
#pragma unroll
    for (int bi = 0; bi < 4; ++bi) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const uint32_t row = l.wy * 128 + bi * 32 + c_row(r, l.g);
        const float2 sr = st_rows[row];
        const uint32_t li = tr_p * kT + row;
#pragma unroll
        for (int bj = 0; bj < 4; ++bj) {
          const uint32_t lj = tc_p * kT + l.wx * 128 + bj * 32 + l.lr;
          // cuking.cu:199 plus the tile padding
          const bool valid = li < a.geo.num_rows && lj < a.geo.num_cols &&
                             a.i_begin + li < a.j_begin + lj;
          // u_i + u_j - 2 q  <  t min(|H_i|, |H_j|) + margin   ("Offset code" above:
          // u~_i - 8 acc first, below 2^24 in magnitude, then u~_j)
          const float x_lb = fmaf(-8.f, acc[bi][bj][r], sr.x) + sc[bj].x;
          const bool cand = valid && x_lb < fminf(sr.y, sc[bj].y);
          const unsigned long long b = __ballot(cand);
          if (b != 0) {  // wave-uniform
            if (pass == 0) {
              total += (uint32_t)__popcll(b);
            } else {
              const uint32_t before = __builtin_amdgcn_mbcnt_hi(
                  (uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
              if (cand) a.cand_list[base + run + before] = make_uint2(li, lj);
              run += (uint32_t)__popcll(b);
            }
          }
        }
      }
    }
    if (pass == 0) {
      if (total == 0) break;  // wave-uniform: the usual case
      bool dense = total > a.quadrant_cap;
      if (!dense) {
        uint32_t got = 0;
        if (l.lane == 0) {
          got = relaxed_add(a.filter_ctrl, total);
          // (running total since the scratch was allocated: "filter_candidates")
          relaxed_add(a.filter_totals + kTotalCand, total);
        }
        base = (uint32_t)__builtin_amdgcn_readfirstlane(got);
        if (base >= a.cand_cap || total > a.cand_cap - base) {
          // list full: the slots taken (if any) must not be read as pairs
          for (uint32_t k = base + l.lane; k < a.cand_cap; k += 64)
            a.cand_list[k] = make_uint2(kNoPair, kNoPair);
          dense = true;
        }
      }
      if (dense) {
        if (l.lane == 0) {
          const uint32_t slot = relaxed_add(a.filter_ctrl + kCtrlDense, 1u);
          if (slot < a.dense_cap) a.dense_list[slot] = make_uint2(2 * t.tr + l.wy, 2 * t.tc + l.wx);
          relaxed_add(a.filter_totals + kTotalDense, 1ull);
        }
        break;
      }
    }
  }
}

// ---- The k loop's statements: macros over filter_tile()'s locals (acc, FA / FB / RAW, mT / mA /
// scaleB, lane16 / row_off / col_off, row_bytes, and a segment's running pa, buf, step).
// One LDS-DMA request: lane l's 16 bytes of SRC + OFF land at DST + OFF + 16 l
// (the immediate offset moves source and destination alike).
#define F_ISSUE(SRC, DST, OFF)                                                 \
  asm volatile("s_mov_b32 m0, %0\n\t"                                          \
               "s_nop 0\n\t"                                                   \
               "global_load_lds_dwordx4 %1, %2 offset:" #OFF                   \
               :                                                               \
               : "s"(DST), "v"(lane16), "s"(SRC)                               \
               : "memory", "m0")
// The four requests of unit c of the stage `pa` names.
#define F_ISSUE4(PA, C)                                                        \
  {                                                                            \
    const char *src_ = (PA).src + (C) * row_bytes;                             \
    const uint32_t dst_ = (PA).dst + (C) * (kSliceU4 * 16);                    \
    F_ISSUE(src_, dst_, 0);                                                    \
    F_ISSUE(src_, dst_, 1024);                                                 \
    F_ISSUE(src_, dst_, 2048);                                                 \
    F_ISSUE(src_, dst_, 3072);                                                 \
  }
#define F_READ(K, BUF, C)                                                      \
  RAW[K] = lds[(BUF) * kStageU4 + ((K) < 4 ? row_off : col_off) + (C) * kSliceU4 + ((K) & 3) * 32];
// (plain ANDs: nothing but data orders them against the MFMAs, and
// left alone the compiler builds every fragment right behind its LDS read, i.e.
// waits for the read it has just issued.  The empty asm statements tie a build
// to the place it is written in: not above the pin of its input, not below the
// pin of its result -- as in king_mfma.hip.)
#define F_PIN4(W) asm volatile("" : "+v"((W).x), "+v"((W).y), "+v"((W).z), "+v"((W).w));
#define F_PINF(F) asm volatile("" : "+v"((F)[0]), "+v"((F)[1]), "+v"((F)[2]), "+v"((F)[3]));
// Set B of word K: bits 2-3 of every nibble as they are.
#define F_BUILD_B(NXT, K)                                                      \
  F_PIN4(RAW[K])                                                               \
  if ((K) < 4) {                                                               \
    FA[NXT][(K) & 3] = tfrag(RAW[K], mT);                                      \
    F_PINF(FA[NXT][(K) & 3])                                                   \
  } else {                                                                     \
    FB[NXT][(K) & 3] = tfrag(RAW[K], mT);                                      \
    F_PINF(FB[NXT][(K) & 3])                                                   \
  }
// Set A of word K: bits 0-1 of every nibble as they are (1 + T: 0 / 0.5 / 1.0 in fp4).
#define F_BUILD_A(NXT, K)                                                      \
  F_PIN4(RAW[K])                                                               \
  if ((K) < 4) {                                                               \
    FA[NXT][(K) & 3] = tfrag(RAW[K], mA);                                      \
    F_PINF(FA[NXT][(K) & 3])                                                   \
  } else {                                                                     \
    FB[NXT][(K) & 3] = tfrag(RAW[K], mA);                                      \
    F_PINF(FB[NXT][(K) & 3])                                                   \
  }
// (fragment set 0 holds set B: the scaled instruction; fragment set 1 holds set A)
#define F_MMA(CUR, BI, BJ)                                                     \
  acc[BI][BJ] = (CUR) == 0 ? mma_scaled(FA[CUR][BI], FB[CUR][BJ], acc[BI][BJ], scaleB) \
                           : mma(FA[CUR][BI], FB[CUR][BJ], acc[BI][BJ]);
#define F_BAR __builtin_amdgcn_sched_barrier(0);
// Slice B of unit c (fragment set CUR): 16 MFMAs; in their gaps the set-A
// fragments of the same words (4 VALU per fragment, in every second gap: the
// gaps that take a request stay free) and two requests.
#define F_SLICE_B(CUR, NXT, PA, DC, OFF0, OFF1)                                \
  {                                                                            \
    const char *src_ = (PA).src + (DC) * row_bytes;                            \
    const uint32_t dst_ = (PA).dst + (DC) * (kSliceU4 * 16);                   \
    F_ISSUE(src_, dst_, OFF0);                                                 \
    F_MMA(CUR, 0, 0) F_BAR                                                     \
    F_BUILD_A(NXT, 0) F_MMA(CUR, 0, 1) F_BAR                                   \
    F_MMA(CUR, 0, 2) F_BAR                                                     \
    F_BUILD_A(NXT, 1) F_MMA(CUR, 0, 3) F_BAR                                   \
    F_MMA(CUR, 1, 0) F_BAR                                                     \
    F_BUILD_A(NXT, 2) F_MMA(CUR, 1, 1) F_BAR                                   \
    F_MMA(CUR, 1, 2) F_BAR                                                     \
    F_BUILD_A(NXT, 3) F_MMA(CUR, 1, 3) F_BAR                                   \
    F_ISSUE(src_, dst_, OFF1);                                                 \
    F_MMA(CUR, 2, 0) F_BAR                                                     \
    F_BUILD_A(NXT, 4) F_MMA(CUR, 2, 1) F_BAR                                   \
    F_MMA(CUR, 2, 2) F_BAR                                                     \
    F_BUILD_A(NXT, 5) F_MMA(CUR, 2, 3) F_BAR                                   \
    F_MMA(CUR, 3, 0) F_BAR                                                     \
    F_BUILD_A(NXT, 6) F_MMA(CUR, 3, 1) F_BAR                                   \
    F_MMA(CUR, 3, 2) F_BAR                                                     \
    F_BUILD_A(NXT, 7) F_MMA(CUR, 3, 3) F_BAR                                   \
  }
// Slice A of a unit (fragment set CUR): 16 MFMAs; in the gaps of the first
// eight the LDS reads of the NEXT unit's words (RBUF, RC; behind the stage
// hand-over if SYNC: that read is the first of a new stage) and two requests,
// in the gaps of the last eight that unit's set-B fragments.
#define F_SLICE_A(CUR, NXT, RBUF, RC, SYNC, PA, DC, OFF0, OFF1)                \
  {                                                                            \
    if (SYNC) {                                                                \
      __builtin_amdgcn_s_waitcnt(vmcnt_imm(kSyncVm));                          \
      __syncthreads();                                                         \
    }                                                                          \
    const char *src_ = (PA).src + (DC) * row_bytes;                            \
    const uint32_t dst_ = (PA).dst + (DC) * (kSliceU4 * 16);                   \
    F_READ(0, RBUF, RC) F_READ(1, RBUF, RC)                                    \
    F_ISSUE(src_, dst_, OFF0);                                                 \
    F_MMA(CUR, 0, 0) F_MMA(CUR, 0, 1) F_BAR                                    \
    F_READ(2, RBUF, RC) F_READ(3, RBUF, RC)                                    \
    F_MMA(CUR, 0, 2) F_MMA(CUR, 0, 3) F_BAR                                    \
    F_READ(4, RBUF, RC) F_READ(5, RBUF, RC)                                    \
    F_ISSUE(src_, dst_, OFF1);                                                 \
    F_MMA(CUR, 1, 0) F_MMA(CUR, 1, 1) F_BAR                                    \
    F_READ(6, RBUF, RC) F_READ(7, RBUF, RC)                                    \
    F_MMA(CUR, 1, 2) F_MMA(CUR, 1, 3) F_BAR                                    \
    F_BUILD_B(NXT, 0) F_MMA(CUR, 2, 0) F_BAR                                   \
    F_BUILD_B(NXT, 1) F_MMA(CUR, 2, 1) F_BAR                                   \
    F_BUILD_B(NXT, 2) F_MMA(CUR, 2, 2) F_BAR                                   \
    F_BUILD_B(NXT, 3) F_MMA(CUR, 2, 3) F_BAR                                   \
    F_BUILD_B(NXT, 4) F_MMA(CUR, 3, 0) F_BAR                                   \
    F_BUILD_B(NXT, 5) F_MMA(CUR, 3, 1) F_BAR                                   \
    F_BUILD_B(NXT, 6) F_MMA(CUR, 3, 2) F_BAR                                   \
    F_BUILD_B(NXT, 7) F_MMA(CUR, 3, 3) F_BAR                                   \
  }
// k-step s requests stage s + kStages - 1 into the buffer stage s - 1 left: every
// wavefront finished reading it before the hand-over of k-step s - 1.  The
// hand-over of k-step s (stage s + 1 must have landed) comes in its last slice:
// in flight then may be the stages after s + 1 and the requests of the newest one
// that the slices before the last have issued (kSyncVm: 2 x 8 + 6 = 22).
#define F_KSTEP                                                                \
  {                                                                            \
    const uint32_t nbuf = buf == kStages - 1 ? 0 : buf + 1;                    \
    F_SLICE_B(0, 1, pa, 0, 0, 1024)                                            \
    F_SLICE_A(1, 0, buf, 1, false, pa, 0, 2048, 3072)                          \
    F_SLICE_B(0, 1, pa, 1, 0, 1024)                                            \
    F_SLICE_A(1, 0, nbuf, 0, true, pa, 1, 2048, 3072)                          \
    pa = addr_next(pa, step + kStages, buf);                                   \
    buf = nbuf;                                                                \
    ++step;                                                                    \
  }
// The k-step this tile has reached, for the tiles of the XCD that start next -- counted
// around the tile's ring (a head lap: around the head; behind its one turn, in the tail, a
// tile says nothing: it would pull newcomers out of the head) (one lane of
// one wavefront: the branch is scalar, the lane mask is set by hand -- a divergent branch
// here makes the compiler treat the segment loop as divergent)
#define F_PUBLISH(STEPS)                                                       \
  if (a.rotate == 1 && wave == 0 && (STEPS) <= ring) {                         \
    const uint32_t now_ = (uint32_t)__builtin_amdgcn_s_memrealtime();          \
    const unsigned long long val_ =                                            \
        ((unsigned long long)(start_abs + (STEPS)) << 32) | now_;              \
    /* ticks per k-step x 16, once the tile has made enough of them to tell   \
       (16: the head of the shortest bitset whose tiles lap says so too) */    \
    const uint32_t t16_ = (STEPS) >= 16 ? (now_ - t_start) * 16u / (STEPS) : 0u; \
    const uint32_t zero_ = 0;                                                  \
    unsigned long long save_;                                                  \
    asm volatile("s_mov_b64 %0, exec\n\t"                                      \
                 "s_mov_b64 exec, 1\n\t"                                       \
                 "global_store_dwordx2 %1, %2, %3\n\t"                         \
                 "s_mov_b64 exec, %0"                                          \
                 : "=&s"(save_)                                                \
                 : "v"(zero_), "v"(val_), "s"(pos_word)                        \
                 : "memory");                                                  \
    if (t16_ != 0)                                                             \
      asm volatile("s_mov_b64 %0, exec\n\t"                                    \
                   "s_mov_b64 exec, 1\n\t"                                     \
                   "global_store_dword %1, %2, %3\n\t"                         \
                   "s_mov_b64 exec, %0"                                        \
                   : "=&s"(save_)                                              \
                   : "v"(zero_), "v"(t16_), "s"(ticks_word)                    \
                   : "memory");                                                \
  }

// One tile (or one piece of the k range of a tile) of the launch: what workgroup `wg` of a
// grid of one workgroup per tile does -- the phases above around the k loop.  Every return
// but the epilogue's is uniform across the workgroup.  lds: [kStages][side][k-half][unit][256].
__device__ __forceinline__ void filter_tile(const TiledArgs &a, const uint32_t wg, uint4 *const lds) {
  Tile tile;
  if (!take_tile(a, wg, lds, &tile)) return;
  const Lanes ln = lanes_of_thread();
  uint32_t xcd_pos = 0, order_share = 0;
  if (!tile.split && a.tile_done != nullptr &&
      launch_verdict(a, wg, lds, &xcd_pos, &order_share))
    return;
  // k-steps of 256 sites: all of them, or this piece's share
  const uint32_t all_steps = a.geo.k_words / (4 * kUnits);
  // (wave-uniform, but divisions run in vector registers: pinned to SGPRs for the
  //  request addresses)
  const uint32_t k_first = __builtin_amdgcn_readfirstlane(
      tile.split ? tile.part * all_steps / a.fsplit_parts : 0u);
  const uint32_t num_steps = __builtin_amdgcn_readfirstlane(
      tile.split ? (tile.part + 1) * all_steps / a.fsplit_parts - k_first : all_steps);
  const CheckPlan plan = plan_checks(a, tile, xcd_pos, order_share, all_steps, num_steps);

  // --- the k loop: acc = (q + n_A + S_i + S_j) / 4 of the tile's pairs ("Offset code" above)
  // (the names the F_* macros and the segment loop below use)
  const uint32_t wave = ln.wave, chk0 = plan.chk0, chk1 = plan.chk1;
  const uint32_t k0 = plan.k0, wrap = plan.wrap, ring = plan.ring, start_abs = plan.start_abs;
  uint32_t lane16 = ln.lane * 16;
  const uint32_t s_stride = a.geo.s_stride;
  const uint4 *g_rows = a.t2 + (uint64_t)tile.tr * kT;
  const uint4 *g_cols = a.t2 + a.geo.col_base + (uint64_t)tile.tc * kT;

  // The masks of the two site sets of a T2 word and the scale of set B (king_common.h:
  // +-2.0 x 2^-2 per operand, so that a set-B product weighs 1/4 like a set-A product),
  // set once and pinned.
  uint32_t mT, mA;
  asm volatile("s_mov_b32 %0, 0xcccccccc" : "=s"(mT));
  asm volatile("s_mov_b32 %0, 0x33333333" : "=s"(mA));
  int scaleB;
  asm volatile("v_mov_b32 %0, 0x7d7d7d7d" : "=v"(scaleB));

  // LDS-DMA: wavefront (side, k-half) fetches that quarter of a stage: 2 units x
  // 4 runs of 64 samples, 1 KiB each.  Unit c of k-step s, k-half h is unit
  // 4 s + 2 h + c of the T2 layout (the order of the sites inside k does not
  // matter as long as rows and columns agree); every unit feeds TWO slices of 64
  // sites per k-half: its bits 2-3 (set B) and its bits 0-1 (set A).
  const uint32_t dma_side = wave >> 1, dma_h = wave & 1;
  const uint32_t row_bytes = s_stride * 16;  // one unit of the layout
  const char *const g_wave = reinterpret_cast<const char *>(
      (dma_side ? g_cols : g_rows) + ((uint64_t)2 * kUnits * k_first + kUnits * dma_h) * s_stride);
  const uint32_t l_wave = (uint32_t)(uintptr_t)(lds_void_ptr)(
      lds + ((dma_side * 2 + dma_h) * kUnits) * kSliceU4);
  struct Addr { const char *src; uint32_t dst; };  // of unit 0; unit 1: + row_bytes, + 4 KiB
  const uint32_t kstep_bytes = 2 * kUnits * row_bytes;
  // The pipeline runs over one SEGMENT of the piece's k-steps at a time (one segment,
  // unless the tile has check points): `seg_src` is the wavefront's first request
  // of the segment, `seg_steps` its k-steps.
  const char *seg_src = g_wave;
  uint32_t seg_steps = num_steps;
  // (a rotated tile: k-step `seg_wrap` of the segment is the bitset's FIRST again --
  //  `ring` k-steps back; 32-bit scalar selects and one signed product: a select between
  //  two 64-bit addresses goes through vector registers, which the scalar pins cannot take)
  uint32_t seg_wrap = 0xFFFFFFFFu;
  auto addr_of = [&](uint32_t step, uint32_t buf) {
    Addr pa;
    if (step >= seg_steps) step = seg_steps - 1;  // clamped repeats (see king_mfma.hip)
    const int32_t rel = (int32_t)step - (int32_t)(step >= seg_wrap ? ring : 0u);
    pa.src = seg_src + (int64_t)rel * (int64_t)kstep_bytes;
    pa.dst = l_wave + buf * (kStageU4 * 16);
    asm volatile("" : "+s"(pa.src), "+s"(pa.dst));
    return pa;
  };
  auto addr_next = [&](const Addr &cur, uint32_t step, uint32_t buf) {
    Addr pa;
    const int32_t adv = (int32_t)(step < seg_steps ? 1u : 0u) -
                        (int32_t)(step == seg_wrap ? ring : 0u);
    pa.src = cur.src + (int64_t)adv * (int64_t)kstep_bytes;
    pa.dst = l_wave + buf * (kStageU4 * 16);
    asm volatile("" : "+s"(pa.src), "+s"(pa.dst));
    return pa;
  };

  v16f acc[4][4] = {};

  // This lane's operand words inside a stage (uint4 units).
  uint32_t row_off = ((0 * 2 + ln.g) * kUnits) * kSliceU4 + ln.wy * 128 + ln.lr;
  uint32_t col_off = ((1 * 2 + ln.g) * kUnits) * kSliceU4 + ln.wx * 128 + ln.lr;
  asm volatile("" : "+v"(row_off), "+v"(col_off), "+v"(lane16));
  v8i FA[2][4], FB[2][4];  // T fragments [slice parity][block]
  uint4 RAW[8];            // the words of one unit: rows 0-3, columns 4-7

  unsigned long long *const pos_word =
      reinterpret_cast<unsigned long long *>(a.filter_ctrl + kCtrlPos) +
      (wg & 7) * kPosSlots + ((wg >> 3) & (kPosSlots - 1));
  uint32_t *const ticks_word = a.filter_ctrl + kCtrlStepTicks + (wg & 7);
  // (the first request of the tile goes out about now)
  const uint32_t t_start = a.rotate == 1 ? (uint32_t)__builtin_amdgcn_s_memrealtime() : 0u;

  uint32_t seg_first = 0;  // k-steps of the piece behind us
  Leave left = kStays;
#pragma nounroll
  while (true) {
    uint32_t seg_end = num_steps;
    if (chk1 > seg_first) seg_end = chk1;
    if (chk0 > seg_first) seg_end = chk0;
    seg_end = __builtin_amdgcn_readfirstlane(seg_end);
    seg_steps = seg_end - seg_first;
    // (the segment's first k-step of the bitset: behind the end of the ring it counts from
    //  0 again; a segment that holds the end goes around it without a pause; behind one turn
    //  of a head lap's ring, in the tail, the tile's k-steps are the bitset's)
    const uint32_t seg_k = seg_first >= ring                ? seg_first
                           : seg_first >= wrap && wrap != 0 ? seg_first - wrap
                                                            : k0 + seg_first;
    seg_src = g_wave + (uint64_t)seg_k * kstep_bytes;
    seg_wrap = __builtin_amdgcn_readfirstlane(
        wrap > seg_first && wrap < seg_end ? wrap - seg_first : 0xFFFFFFFFu);
    asm volatile("" : "+s"(seg_src), "+s"(seg_steps), "+s"(seg_wrap));

    // Stages 0 .. 3 of the segment requested, stage 0 landed.
#pragma unroll
    for (int st = 0; st < kStages - 1; ++st) {
      const Addr p0 = addr_of(st, st);
      F_ISSUE4(p0, 0)
      F_ISSUE4(p0, 1)
    }
    __builtin_amdgcn_s_waitcnt(vmcnt_imm((kStages - 2) * kStageReqs));
    __syncthreads();
    // unit 0 of stage 0, set B
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      F_READ(k, 0, 0)
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      F_BUILD_B(0, k)
    }
    uint32_t buf = 0;  // buffer of the k-step being multiplied
    Addr pa = addr_of(kStages - 1, kStages - 1);
    uint32_t step = 0;
    while (step + 1 < seg_steps) {
      F_KSTEP
      F_KSTEP
    }
    if (step < seg_steps) F_KSTEP
    // The clamped repeats of the last stage must have landed before the stages
    // become the check's or the epilogue's scratch.
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    __syncthreads();
    F_PUBLISH(seg_end)
    if (seg_end == num_steps) break;

    // --- the check behind k-step seg_end of the tile
    left = check_sweep(a, tile, plan, acc, lds, seg_end == chk0, all_steps);
    // The tile leaves (uniform; nothing is in flight; the book-keeping follows behind
    // the loop: a divergent branch on the way out makes the compiler treat the whole
    // loop as divergent, request addresses and all).
    if (left != kStays) break;
    seg_first = seg_end;
  }

  if (leave_early(a, tile, plan, left)) return;
  if (tile.split && !reduce_pieces(a, tile, acc, lds)) return;
  emit_candidates(a, tile, plan, acc, lds, left == kLeftEmit);
}
#undef F_KSTEP
#undef F_SLICE_A
#undef F_SLICE_B
#undef F_BAR
#undef F_MMA
#undef F_BUILD_A
#undef F_BUILD_B
#undef F_PIN4
#undef F_PINF
#undef F_READ
#undef F_ISSUE4
#undef F_ISSUE
#undef F_PUBLISH

__global__ __launch_bounds__(256, 1) void king_filter_kernel(const TiledArgs a) {
  extern __shared__ uint4 lds[];
  filter_tile(a, blockIdx.x, lds);
}

// One wavefront per candidate pair: the reference's six sums (cuking.cu:219-239)
// straight from the bitset, kinship, threshold, record (cuking.cu:284-313).
__global__ __launch_bounds__(256) void king_refine_kernel(const TiledArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  uint32_t count = *a.filter_ctrl;
  if (count > a.cand_cap) count = a.cand_cap;
  const uint32_t n = a.words_per_sample / 2;
  const uint32_t stride = gridDim.x * 4;
  for (uint32_t p = blockIdx.x * 4 + (threadIdx.x >> 6); p < count; p += stride) {
    const uint2 e = a.cand_list[p];
    if (e.x == kNoPair) continue;  // (uniform: a slot of a quadrant that went dense)
    // (plane indices of the pair -> the stored samples behind them, king_common.h `perm`)
    const uint32_t off_i = a.perm != nullptr ? a.perm[e.x] : e.x;
    const uint32_t off_j = a.perm != nullptr ? a.perm[a.geo.col_base + e.y]
                                             : (a.geo.diag ? e.y : a.geo.num_rows + e.y);
    const uint64_t *het_i_w = a.bits + (uint64_t)off_i * a.words_per_sample;
    const uint64_t *alt_i_w = het_i_w + n;
    const uint64_t *het_j_w = a.bits + (uint64_t)off_j * a.words_per_sample;
    const uint64_t *alt_j_w = het_j_w + n;
    uint32_t s_het_i = 0, s_het_j = 0, s_both = 0, s_opp = 0, s_conc = 0, s_shared = 0;
    // words per lane and plane requested before any is counted: the planes of an arbitrary
    // pair are cold, a trip is one memory latency (100k sites: 4 trips; 21 us for the 770
    // candidates of configs[1] with 4 words in flight)
    constexpr uint32_t kAhead = 8;
    for (uint32_t w0 = 0; w0 < n; w0 += 64 * kAhead) {
      uint64_t hi[kAhead], ai[kAhead], hj[kAhead], aj[kAhead];
#pragma unroll
      for (uint32_t k = 0; k < kAhead; ++k) {
        const uint32_t w = w0 + 64 * k + lane;
        const bool in = w < n;  // beyond the plane: missing
        hi[k] = in ? het_i_w[w] : ~0ull;
        ai[k] = in ? alt_i_w[w] : ~0ull;
        hj[k] = in ? het_j_w[w] : ~0ull;
        aj[k] = in ? alt_j_w[w] : ~0ull;
      }
#pragma unroll
      for (uint32_t k = 0; k < kAhead; ++k) {
        const uint64_t ri = ~(hi[k] | ai[k]), rj = ~(hj[k] | aj[k]);
        const uint64_t defined = ~((hi[k] & ai[k]) | (hj[k] & aj[k]));
        s_het_i += __popcll(hi[k] & defined);
        s_het_j += __popcll(hj[k] & defined);
        s_both += __popcll(hi[k] & hj[k] & defined);
        s_opp += __popcll(((ri & aj[k]) | (ai[k] & rj)) & defined);
        s_conc += __popcll(((ri & rj) | (ai[k] & aj[k])) & defined);
        s_shared += __popcll(defined);
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      s_het_i += __shfl_xor(s_het_i, off);
      s_het_j += __shfl_xor(s_het_j, off);
      s_both += __shfl_xor(s_both, off);
      s_opp += __shfl_xor(s_opp, off);
      s_conc += __shfl_xor(s_conc, off);
      s_shared += __shfl_xor(s_shared, off);
    }
    if (lane == 0) {
      const float kin = king_kinship(s_het_i, s_het_j, s_both, s_opp);
      if (kin > a.kin_threshold) {
        const uint32_t ibs0 = s_opp, ibs2 = s_conc + s_both;
        const uint32_t gi = a.i_begin + off_i;
        const uint32_t gj = a.geo.diag ? a.j_begin + off_j : a.j_begin + (off_j - a.geo.num_rows);
        emit_result(gi < gj ? gi : gj, gi < gj ? gj : gi, kin, ibs0, s_shared - ibs0 - ibs2, ibs2,
                    a.max_results, a.results, a.result_index, a.result_overflow);
      }
    }
  }
}

// The counting form of king_refine_kernel (TiledArgs::rel_counts, a kernel of its own so that
// the record form stays as it is): one wavefront per candidate pair, only the four sums
// kinship needs (cuking.cu:232-235), the same king_kinship() float a record carries, its band
// among the call's thresholds (king_kin_summary.h rel_band) and one atomic per end of the
// pair, at the STORED samples' rows of rel_counts.  No record, no IBS sums.
__global__ __launch_bounds__(256) void king_refine_count_kernel(const TiledArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  uint32_t count = *a.filter_ctrl;
  if (count > a.cand_cap) count = a.cand_cap;
  const uint32_t n = a.words_per_sample / 2;
  const uint32_t stride = gridDim.x * 4;
  for (uint32_t p = blockIdx.x * 4 + (threadIdx.x >> 6); p < count; p += stride) {
    const uint2 e = a.cand_list[p];
    if (e.x == kNoPair) continue;  // (uniform: a slot of a quadrant that went dense)
    const uint32_t off_i = a.perm != nullptr ? a.perm[e.x] : e.x;
    const uint32_t off_j = a.perm != nullptr ? a.perm[a.geo.col_base + e.y]
                                             : (a.geo.diag ? e.y : a.geo.num_rows + e.y);
    const uint64_t *het_i_w = a.bits + (uint64_t)off_i * a.words_per_sample;
    const uint64_t *alt_i_w = het_i_w + n;
    const uint64_t *het_j_w = a.bits + (uint64_t)off_j * a.words_per_sample;
    const uint64_t *alt_j_w = het_j_w + n;
    uint32_t s_het_i = 0, s_het_j = 0, s_both = 0, s_opp = 0;
    constexpr uint32_t kAhead = 8;  // (as in king_refine_kernel)
    for (uint32_t w0 = 0; w0 < n; w0 += 64 * kAhead) {
      uint64_t hi[kAhead], ai[kAhead], hj[kAhead], aj[kAhead];
#pragma unroll
      for (uint32_t k = 0; k < kAhead; ++k) {
        const uint32_t w = w0 + 64 * k + lane;
        const bool in = w < n;  // beyond the plane: missing
        hi[k] = in ? het_i_w[w] : ~0ull;
        ai[k] = in ? alt_i_w[w] : ~0ull;
        hj[k] = in ? het_j_w[w] : ~0ull;
        aj[k] = in ? alt_j_w[w] : ~0ull;
      }
#pragma unroll
      for (uint32_t k = 0; k < kAhead; ++k) {
        const uint64_t ri = ~(hi[k] | ai[k]), rj = ~(hj[k] | aj[k]);
        const uint64_t defined = ~((hi[k] & ai[k]) | (hj[k] & aj[k]));
        s_het_i += __popcll(hi[k] & defined);
        s_het_j += __popcll(hj[k] & defined);
        s_both += __popcll(hi[k] & hj[k] & defined);
        s_opp += __popcll(((ri & aj[k]) | (ai[k] & rj)) & defined);
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      s_het_i += __shfl_xor(s_het_i, off);
      s_het_j += __shfl_xor(s_het_j, off);
      s_both += __shfl_xor(s_both, off);
      s_opp += __shfl_xor(s_opp, off);
    }
    if (lane == 0) {
      const uint32_t band = rel_band(a.rel_thr, a.rel_num, king_kinship(s_het_i, s_het_j, s_both, s_opp));
      if (band != kRelNoBand) {
        atomicAdd(a.rel_counts + (size_t)off_i * a.rel_num + band, 1u);
        atomicAdd(a.rel_counts + (size_t)off_j * a.rel_num + band, 1u);
      }
    }
  }
}

}  // namespace

static std::atomic<uint32_t> g_check_min_steps{64};
void set_filter_check_min_steps(uint32_t steps) { g_check_min_steps.store(steps); }
uint32_t filter_check_min_steps() { return g_check_min_steps.load(); }

hipError_t launch_sample_stats(const uint64_t *d_bit_sets, uint32_t words_per_sample,
                               const PlaneGeometry &geo, uint4 *d_planes, uint32_t s_begin,
                               uint32_t s_end, hipStream_t stream) {
  // (in stored order, into the arrays the sample order is built from: king_sort.hip puts
  //  them into plane order)
  return launch_sample_stats_to(d_bit_sets, words_per_sample, geo, stats_arrays(geo, d_planes),
                                s_begin, s_end, stream);
}

hipError_t launch_sample_stats_to(const uint64_t *d_bit_sets, uint32_t words_per_sample,
                                  const PlaneGeometry &geo, const SampleStatsArrays &to,
                                  uint32_t s_begin, uint32_t s_end, hipStream_t stream) {
  if (s_end > geo.s_stride) s_end = geo.s_stride;
  if (s_begin >= s_end) return hipSuccess;
  float2 *stats = to.stats;
  float *prefix = to.cum;
  unsigned long long *sums = to.sums;
  uint32_t *steps = to.steps;
  CheckWords cw;
  const uint32_t all_steps = geo.k_words / 8;  // k-steps of 256 sites
  if (all_steps > kStatsMaxSteps) return hipErrorInvalidValue;
  for (uint32_t k = 0; k < kNumCheckShares; ++k)
    cw.w[k] = check_step_of(all_steps, k, g_check_min_steps.load());
  sample_stats_kernel<<<dim3((s_end - s_begin + 3) / 4), dim3(256), 0, stream>>>(
      d_bit_sets, words_per_sample, geo, stats, prefix, sums, steps, cw, s_begin, s_end);
  return hipGetLastError();
}

hipError_t launch_filter(const TiledArgs &args, const LaunchSwitches &switches, uint64_t num_tiles,
                         hipStream_t stream) {
  if ((uint64_t)args.geo.k_words * 32 > kMfmaN4MaxSites || args.filter_ctrl == nullptr ||
      args.cand_list == nullptr || args.dense_list == nullptr || args.sample_stats == nullptr)
    return hipErrorInvalidValue;
  const bool count = switches.form == kFormRelCounts;  // the counting form of the exact kernels
  if (!count && switches.form != kFormRecords) return hipErrorInvalidValue;
  if (count && (args.rel_counts == nullptr || args.rel_num == 0 ||
                args.rel_num > CUKING_REL_THRESHOLDS_MAX))
    return hipErrorInvalidValue;
  hipError_t e = allow_dynamic_lds<king_filter_kernel>(kFilterLdsBytes);
  if (e != hipSuccess) return e;
  uint64_t cap = max_blocks_per_launch(256);
  if (cap > kFilterChunkTiles) cap = kFilterChunkTiles;
  // (a chunk's quadrants must fit the dense list)
  if (cap > args.dense_cap / 4) cap = args.dense_cap / 4;
  if (cap == 0) return hipErrorInvalidValue;
  const uint32_t wgs = args.split_wgs != 0 ? args.split_wgs : 256;  // one per CU
  const bool checks = args.tile_done != nullptr;
  // Site order: a tile never wraps around the end of the sites (from the middle of a
  // descending order the weight of [p, p + e) takes MORE k-steps than stored order: 0.90 of
  // them on the flat spectrum, against 0.875).  Where the caller allows it (site_lap:
  // "filter_site_order" 2, and -1 as king_common.h kSiteOrderAutoLap says) a launch that would
  // rotate a stored-order layout rotates its tiles inside the head of the order instead
  // (plan_checks, "head lap"); otherwise the rotation is off and the launch pays the L2 cost
  // of tiles that all start at the first site (profiles/r04_l2_probe.txt: hit rate 0.41
  // against 0.75, about 3.5 % of the clock).  The test hooks always take the lap.
  LaunchSwitches sw = switches;
  if (args.site_curve != nullptr && sw.rotate == 1 && args.site_lap == 0) sw.rotate = 0;
  const bool can_split = args.fsplit_slabs != nullptr && args.fsplit_tickets != nullptr;
  for (uint64_t done = 0; done < num_tiles;) {
    const FilterPlan p = filter_plan(num_tiles - done, cap, wgs, args.geo.k_words / 8, checks,
                                     can_split, kFilterSplitSlabs, sw);
    // (the chunk's control words and, directly behind them, its tile flags: one memset)
    e = hipMemsetAsync(args.filter_ctrl, 0, kCtrlChunkBytes + (checks ? p.n : 0), stream);
    if (e != hipSuccess) return e;
    TiledArgs chunk = args;  // the chunk's tiles, no mode set: what the exact kernel starts from
    chunk.tile_begin = args.tile_begin + done;
    TiledArgs a = chunk;
    a.check0 = p.check0;
    a.check1 = p.check1;
    a.rotate = p.rotate;
    a.launch_tiles = p.whole.launch_tiles;
    a.xcd_chunk = p.whole.xcd_chunk;
    a.dyn_tiles = p.whole.dyn_tiles;
    a.dyn_wgs = p.whole.dyn_wgs;
    a.fsplit_parts = p.parts;
    a.fsplit_tile0 = p.fsplit_tile0;
    a.fsplit_first = p.fsplit_first;
    // (the tiles of the remainder pieces never leave early: done as far as the fallback
    //  launch is concerned)
    if (checks && p.rest != 0) {
      e = hipMemsetAsync(args.tile_done + p.fsplit_tile0, 1, p.rest, stream);
      if (e != hipSuccess) return e;
    }
    king_filter_kernel<<<dim3((uint32_t)p.grid), dim3(256), kFilterLdsBytes, stream>>>(a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    // (a relative-counts call: the counting form; so do the two launches below)
    if (count) king_refine_count_kernel<<<dim3(wgs * 4), dim3(256), 0, stream>>>(a);
    else king_refine_kernel<<<dim3(wgs * 4), dim3(256), 0, stream>>>(a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (a.codes_ready != nullptr) {
      // Lazy codes (king_common.h): the four-product kernel's layout for the whole block,
      // if this chunk handed anything to that kernel and the codes are not there yet.
      e = launch_prepare_nibbles(true, false, a.bits, a.words_per_sample, a.geo,
                                 const_cast<uint4 *>(a.planes), a.perm, 0, 0xFFFFFFFFu,
                                 a.filter_ctrl, a.codes_ready, stream);
      if (e != hipSuccess) return e;
      e = launch_mark_codes_ready(a.filter_ctrl, a.codes_ready, stream);
      if (e != hipSuccess) return e;
    }
    // the quadrants that went dense
    e = launch_mfma_list(sw.form, chunk, args.dense_list, args.filter_ctrl + kCtrlDense,
                         args.dense_cap, wgs, stream);
    if (e != hipSuccess) return e;
    if (checks) {
      // The fallback: every tile of the chunk that has not set its flag (it left at
      // check 0, or never started because most quadrants of the launch had gone dense),
      // in the four-product kernel's own order -- if there is any: the gate word.
      TiledArgs f = chunk;
      uint64_t units = p.n;
      to_quadrants(&f, &units);
      e = launch_mfma_gated(sw.form, f, units, args.filter_ctrl + kCtrlGate, args.tile_done,
                            chunk.tile_begin, wgs, stream);
      if (e != hipSuccess) return e;
    }
    done += p.n;
  }
  return hipSuccess;
}

}  // namespace cuking
