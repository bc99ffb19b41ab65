// The sample order of the filter variant's kernel layout (king_common.h, TiledArgs::perm):
// the samples of a prepared range sorted by their share of missing calls.
//
// The slack of the filter's bound is the missingness of the two samples of a pair
// (king_filter.hip: about the missing rate in kinship), so a cohort with a FEW
// low-call-rate samples -- 2 % of the samples at 20 % missing calls is an ordinary exome
// batch effect -- has a few samples whose pairs the bound cannot rule out.  In stored order
// they sit two or three to every 128 x 128 quadrant, and every quadrant of the cohort goes
// to the exact kernel; sorted, they fill the last tile rows and columns and the other 96 %
// of the tiles keep the filter's speed.  The reference has no counterpart (it evaluates
// every pair at constant cost, cuking.cu:216-240).
//
// Steps, per prepared range of plane samples (the whole row / column side of a block, or
// one broadcast chunk of the staged multi-GPU pass -- any tile-aligned range is a valid
// unit, since pairs are enumerated in plane order):
//   1. sample_stats_kernel (king_filter.hip) has left the statistics in STORED order;
//   2. keys: the missing share in 1/64ths (8 bits: one radix pass) -- coarse on purpose: the
//      samples of an ordinary cohort (1 % missing calls, give or take) all get key 0 and
//      the layout IS the stored order;
//   3. a STABLE sort of (key, sample) pairs -- deterministic, and samples of equal share
//      (an ordinary cohort: all of them) keep their stored order;
//   4. perm and the statistics written in plane order -- (u~, |H|) and the cumulative u~,
//      what the filter kernel's pair test reads --; padding samples behind the real ones
//      (kNoSample; u~ = n_A, |H| = 0).
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include "king_common.h"
#include "king_device.h"
#include "king_site_gather.h"

namespace cuking {

namespace {

// Keys of the real samples [begin, begin + n) of a side: stored sample = plane sample
// before the sort.  |M| follows from the statistics: per stored site exactly one of
// hom-and-defined, het, missing, so u = |Y| - |M| = sites - |H| - 2 |M|.
__global__ void sort_keys_kernel(const float2 *__restrict__ tmp_stats, uint32_t begin, uint32_t n,
                                 float stored_sites, uint32_t *__restrict__ keys,
                                 uint32_t *__restrict__ vals) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const float2 st = tmp_stats[begin + p];
  const float missing = 0.5f * (stored_sites - st.y - st.x);
  uint32_t key = (uint32_t)(missing * 64.f / stored_sites);
  keys[p] = key > 255u ? 255u : key;
  vals[p] = begin + p;
}

__global__ void identity_order_kernel(uint32_t begin, uint32_t n, uint32_t *__restrict__ vals) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p < n) vals[p] = begin + p;
}

// Plane samples [begin, end): the first n take the sorted real samples, the rest padding.
__global__ void apply_order_kernel(PlaneGeometry geo, uint32_t begin, uint32_t end, uint32_t n,
                                   const uint32_t *__restrict__ order,
                                   const float2 *__restrict__ tmp_stats,
                                   const float *__restrict__ tmp_prefix,
                                   uint32_t *__restrict__ perm, float2 *__restrict__ stats,
                                   float *__restrict__ prefix) {
  const uint32_t p = begin + blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= end) return;
  if (p - begin >= n) {
    // (T = 0 at every site: u = S = 0, what is left of u~ is n_A, 128 per k-step --
    //  king_filter.hip sample_stats_kernel)
    const uint32_t all_steps = geo.k_words / 8;
    perm[p] = kNoSample;
    stats[p] = make_float2((float)(128u * all_steps), 0.f);
#pragma unroll
    for (uint32_t c = 0; c < kNumCum; ++c)
      prefix[(size_t)c * geo.s_stride + p] = (float)(128u * phase_step(all_steps, c + 1));
    return;
  }
  const uint32_t src = order[p - begin];  // plane sample in stored order
  // the stored sample behind it: rows as they are, columns of an off-diagonal block behind
  // the rows (cuking.cu:171-175)
  perm[p] = (geo.diag || src < geo.rows_padded) ? src : geo.num_rows + (src - geo.col_base);
  // (the pair test's u~ over all sites: the row behind the cumulative ones; |H|)
  stats[p] = make_float2(tmp_prefix[(size_t)kNumCum * geo.s_stride + src], tmp_stats[src].y);
#pragma unroll 7
  for (uint32_t c = 0; c < kNumCum; ++c)
    prefix[(size_t)c * geo.s_stride + p] = tmp_prefix[(size_t)c * geo.s_stride + src];
}

}  // namespace

size_t sort_temp_bytes_for(uint32_t n) {
  size_t bytes = 0;
  uint32_t *nil = nullptr;
  if (n == 0) return 0;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, nil, nil, nil, nil, (int)n, 0, 8);
  return (bytes + 255) / 256 * 256;
}

hipError_t launch_sample_order(const PlaneGeometry &geo, uint32_t words_per_sample,
                               uint4 *d_planes, uint32_t s_begin, uint32_t s_end, bool sort,
                               void *sort_temp, size_t sort_temp_bytes, hipStream_t stream) {
  if (s_end > geo.s_stride) s_end = geo.s_stride;
  if (s_begin >= s_end) return hipSuccess;
  const float2 *tmp_stats = plane_tmp_stats(d_planes, geo);
  const float *tmp_prefix = plane_tmp_prefix(d_planes, geo);
  uint32_t *perm = plane_perm(d_planes, geo);
  float2 *stats = const_cast<float2 *>(plane_stats(d_planes, geo));
  float *prefix = const_cast<float *>(plane_prefix_u(d_planes, geo));
  uint32_t *words = plane_sort_words(d_planes, geo);
  const float stored_sites = 32.f * (float)words_per_sample;  // (what the statistics count over)
  // The sides of the block inside the range: rows [0, rows_padded), columns behind them.
  struct Side { uint32_t begin, end, real_end; };
  Side sides[2];
  int num_sides = 0;
  if (geo.diag) {
    sides[num_sides++] = {0, geo.rows_padded, geo.num_rows};
  } else {
    sides[num_sides++] = {0, geo.rows_padded, geo.num_rows};
    sides[num_sides++] = {geo.col_base, geo.col_base + geo.cols_padded, geo.col_base + geo.num_cols};
  }
  for (int k = 0; k < num_sides; ++k) {
    const uint32_t b = s_begin > sides[k].begin ? s_begin : sides[k].begin;
    const uint32_t e = s_end < sides[k].end ? s_end : sides[k].end;
    if (b >= e) continue;
    const uint32_t real_e = e < sides[k].real_end ? e : sides[k].real_end;
    const uint32_t n = real_e > b ? real_e - b : 0;
    // the sort's four arrays: indexed from the range's first plane sample
    uint32_t *keys_in = words + b, *keys_out = words + geo.s_stride + b;
    uint32_t *vals_in = words + 2 * (size_t)geo.s_stride + b;
    uint32_t *vals_out = words + 3 * (size_t)geo.s_stride + b;
    const uint32_t *order = vals_in;
    if (n != 0) {
      if (sort) {
        sort_keys_kernel<<<dim3((n + 255) / 256), dim3(256), 0, stream>>>(
            tmp_stats, b, n, stored_sites, keys_in, vals_in);
        hipError_t e0 = hipGetLastError();
        if (e0 != hipSuccess) return e0;
        size_t bytes = sort_temp_bytes;
        e0 = hipcub::DeviceRadixSort::SortPairs(sort_temp, bytes, keys_in, keys_out, vals_in,
                                                vals_out, (int)n, 0, 8, stream);
        if (e0 != hipSuccess) return e0;
        order = vals_out;
      } else {
        identity_order_kernel<<<dim3((n + 255) / 256), dim3(256), 0, stream>>>(b, n, vals_in);
        hipError_t e0 = hipGetLastError();
        if (e0 != hipSuccess) return e0;
      }
    }
    apply_order_kernel<<<dim3((e - b + 255) / 256), dim3(256), 0, stream>>>(
        geo, b, e, n, order, tmp_stats, tmp_prefix, perm, stats, prefix);
    hipError_t e1 = hipGetLastError();
    if (e1 != hipSuccess) return e1;
  }
  return hipSuccess;
}

// ---- Site order.  X = sum over the sites of (g_i - g_j)^2 has only non-negative terms and
// KING's sums do not care in which order the sites are visited, as long as every sample uses
// the same one.  The filter kernel's rigorous check (king_filter.hip "Check points") lets a
// tile leave once X over the sites SO FAR has passed the level no record stays under; with
// the sites that contribute most to X of unrelated pairs in front, that happens earlier.
// Steps of a whole-block conversion with the order on:
//   1. site counts (king_site_qc.hip: hom-ref, het, hom-alt, missing per site, one pass);
//   2. weight per site, w = ref het + het alt + 4 ref alt: the sum of (g - g')^2 over the
//      pairs of samples, an exact integer;
//   3. a STABLE descending sort of (weight, site): deterministic for one bitset, ties --
//      monomorphic sites, and the padding of the last word behind them -- keep stored order;
//   4. the bitset once more with every sample's sites in that order (gather_sites_kernel,
//      which counts the statistics of a diagonal block's samples on the way;
//      permute_sites_kernel where "filter_site_gather" says 0), in stream scratch:
//      sample_stats_kernel and the T2 conversion read it instead of the
//      caller's and stay as they are.  Everything that recounts exactly (king_refine_kernel,
//      the four-product kernel's codes) keeps reading the caller's bitset;
//   5. the curve: the weight in front of every phase boundary, and sigma (SiteCurve).
namespace {

constexpr uint32_t kOrderLdsBytes = 64 * 1024;  // what a kernel may ask for without more ado

__global__ void site_keys_kernel(const uint32_t *__restrict__ counts, uint32_t sites,
                                 unsigned long long *__restrict__ keys,
                                 uint32_t *__restrict__ vals) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= sites) return;
  const uint4 c = reinterpret_cast<const uint4 *>(counts)[s];  // ref, het, alt, missing
  const unsigned long long r = c.x, h = c.y, a = c.z;
  keys[s] = r * h + h * a + 4ull * r * a;
  vals[s] = s;
}

// One workgroup per phase: the weight of its sites (in the new order), their share of the
// variance and of the het rate, and their het and missing calls (phase_v: four per phase);
// site_curve_scan_kernel adds the phases up.
__global__ __launch_bounds__(256) void site_curve_kernel(
    const uint32_t *__restrict__ counts, const uint32_t *__restrict__ order, uint32_t sites,
    uint32_t all_steps, unsigned long long *__restrict__ phase_w, double *__restrict__ phase_v) {
  __shared__ unsigned long long w_part[4];
  __shared__ double v_part[4], h_part[4], hc_part[4], mc_part[4];
  const uint32_t x = blockIdx.x;
  const uint32_t begin = 256u * phase_step(all_steps, x), end = 256u * phase_step(all_steps, x + 1);
  unsigned long long w = 0;
  double var = 0., het = 0., hc = 0., mc = 0.;  // (calls: integers below 2^53)
  for (uint32_t d = begin + threadIdx.x; d < end && d < sites; d += 256) {
    const uint4 c = reinterpret_cast<const uint4 *>(counts)[order[d]];
    const double r = c.x, h = c.y, a = c.z, n = r + h + a + (double)c.w;
    const double pairs = 0.5 * n * (n - 1.);
    hc += h;
    mc += (double)c.w;
    if (pairs < 1.) continue;
    w += (unsigned long long)c.x * c.y + (unsigned long long)c.y * c.z +
         4ull * (unsigned long long)c.x * c.z;
    // (g - g')^2 of a random pair: 1 with p1, 4 with p4
    const double p1 = (r * h + h * a) / pairs, p4 = r * a / pairs, mean = p1 + 4. * p4;
    var += p1 + 16. * p4 - mean * mean;
    het += h / n;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    w += __shfl_xor(w, off);
    var += __shfl_xor(var, off);
    het += __shfl_xor(het, off);
    hc += __shfl_xor(hc, off);
    mc += __shfl_xor(mc, off);
  }
  if ((threadIdx.x & 63) == 0) {
    w_part[threadIdx.x >> 6] = w;
    v_part[threadIdx.x >> 6] = var;
    h_part[threadIdx.x >> 6] = het;
    hc_part[threadIdx.x >> 6] = hc;
    mc_part[threadIdx.x >> 6] = mc;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    phase_w[x] = w_part[0] + w_part[1] + w_part[2] + w_part[3];
    phase_v[4 * x] = v_part[0] + v_part[1] + v_part[2] + v_part[3];
    phase_v[4 * x + 1] = h_part[0] + h_part[1] + h_part[2] + h_part[3];
    phase_v[4 * x + 2] = hc_part[0] + hc_part[1] + hc_part[2] + hc_part[3];
    phase_v[4 * x + 3] = mc_part[0] + mc_part[1] + mc_part[2] + mc_part[3];
  }
}

// (128 phases: one thread adds them up)
__global__ __launch_bounds__(64) void site_curve_scan_kernel(
    const unsigned long long *__restrict__ phase_w, const double *__restrict__ phase_v,
    SiteCurve *__restrict__ curve) {
  if (threadIdx.x != 0) return;
  unsigned long long run = 0;
  double var = 0., het = 0., hc = 0., mc = 0.;
  for (uint32_t x = 0; x < kNumPhases; ++x) {
    run += phase_w[x];
    curve->cum[x] = run;
    var += phase_v[4 * x];
    het += phase_v[4 * x + 1];
    hc += phase_v[4 * x + 2];
    mc += phase_v[4 * x + 3];
  }
  curve->het_calls = (unsigned long long)hc;
  curve->missing_calls = (unsigned long long)mc;
  curve->sigma = het > 0. ? (float)(sqrt(var) / (4. * het)) : 1.f;
}

// The gather.  A workgroup stages the two planes of G samples in LDS, interleaved per 32
// sites ({het, hom-alt} halves: one 8-byte read serves both planes), then every wavefront
// assembles runs of 64 output words: lane l looks up the source of destination site
// 64 W + l (`order`, the same for every sample: read once per G samples), fetches its two
// bits, and two ballots ARE output word W of the two planes; lane j keeps word j of the
// run, so that the run goes out as one 512-byte store per plane and sample.
template <int G>
__global__ __launch_bounds__(256) void permute_sites_kernel(
    const uint64_t *__restrict__ bits, uint64_t *__restrict__ out,
    const uint32_t *__restrict__ order, uint32_t num_stored, uint32_t words_per_sample) {
  extern __shared__ uint4 row[];  // [G][plane word]: {het lo, hom lo, het hi, hom hi}
  const uint32_t P = words_per_sample / 2;
  const uint32_t s0 = blockIdx.x * G;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const uint32_t s = s0 + g < num_stored ? s0 + g : num_stored - 1;  // (repeats: not stored)
    const uint64_t *het = bits + (uint64_t)s * words_per_sample, *hom = het + P;
    for (uint32_t w = threadIdx.x; w < P; w += 256) {
      const uint64_t h = het[w], m = hom[w];
      row[g * P + w] = make_uint4((uint32_t)h, (uint32_t)m, (uint32_t)(h >> 32), (uint32_t)(m >> 32));
    }
  }
  __syncthreads();
  const uint2 *half = reinterpret_cast<const uint2 *>(row);  // [G][2 P]: 32 sites of both planes
  for (uint32_t w0 = 64 * wave; w0 < P; w0 += 256) {
    uint64_t oh[G], om[G];
#pragma unroll
    for (int g = 0; g < G; ++g) oh[g] = om[g] = 0;
    // (eight words at a time: their eight reads of `order` go out before the first is used)
    for (uint32_t j0 = 0; j0 < 64 && w0 + j0 < P; j0 += 8) {
      uint32_t src[8];
#pragma unroll
      for (uint32_t k = 0; k < 8; ++k) {
        const uint32_t W = w0 + j0 + k < P ? w0 + j0 + k : P - 1;  // (behind the plane: a repeat, not stored)
        src[k] = order[64 * W + lane];                             // < 64 P
      }
#pragma unroll
      for (uint32_t k = 0; k < 8; ++k) {
        const uint32_t at = src[k] >> 5, bit = 1u << (src[k] & 31);
        const bool mine = lane == j0 + k;
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const uint2 x = half[g * 2 * P + at];
          const uint64_t bh = __ballot((x.x & bit) != 0), bm = __ballot((x.y & bit) != 0);
          if (mine) {
            oh[g] = bh;
            om[g] = bm;
          }
        }
      }
    }
    if (w0 + lane < P) {
#pragma unroll
      for (int g = 0; g < G; ++g) {
        if (s0 + g >= num_stored) continue;
        uint64_t *dst = out + (uint64_t)(s0 + g) * words_per_sample + w0 + lane;
        dst[0] = oh[g];
        dst[P] = om[g];
      }
    }
  }
  // (words_per_sample odd: the word behind the two planes is never read by the conversion)
}

// The byte-wide gather (king_site_gather.h has its arithmetic).  A workgroup stages G samples
// in LDS interleaved per site -- a thread takes source word w of all 2 G rows and turns its
// eight 8 x 8 bit matrices (field x site) around: 64 sites' fields, one 64- or 32-byte
// store --, then every wavefront assembles kGatherBatch destination words at a time:
//   1. lane l reads the field of order[64 W + l] for each word W of the batch (one byte read
//      serves all G samples and both planes) and puts it at [W][l] of the wavefront's tile;
//   2. lane l takes eight neighbouring sites of one word (one 8-byte read), turns the 8 x 8
//      matrix (site x field) around and has byte l & 7 of that word for every field, which
//      goes to [field][word][byte] of the tile (in place: everything is read before anything
//      is written, and the LDS serves a wavefront's requests in order);
//   3. the tile IS the 2 G x kGatherBatch output words: a lane stores G / 2 of them, 16 lanes
//      one 128-byte run of a (sample, plane) row.
// No workgroup barrier behind the staging: a tile belongs to one wavefront.
constexpr uint32_t kGatherLdsMax = 160 * 1024;  // a CU's LDS: one workgroup per CU

__device__ __forceinline__ void wave_lds_order() {
  // (lanes of one wavefront hand data to each other through LDS: the compiler keeps the
  //  accesses in program order, the hardware serves them in that order)
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// STATS: the statistics of sample_stats_kernel (king_filter.hip) for the G samples as well,
// where plane sample = stored sample.  After step 2 the tile holds both planes of 16 words
// of every sample: lane l counts word l & 15 of sample l >> 4 with that kernel's
// expressions -- the totals in registers over the batches, the per-phase sums by integer
// adds in LDS (any order: the same integers) --, and behind the last batch wavefront g does
// sample g's scan and writes with that kernel's float conversions.  The cohort's sums take
// the samples that kernel's grid of `stats_grid` workgroups of four would have added.
struct GatherStatsArgs {
  float2 *stats;
  float *cum;
  unsigned long long *sums;
  uint32_t *steps_out;
  uint32_t s_stride, all_steps, stats_grid;
  uint32_t steps[kNumCheckShares];
};
// LDS behind the tiles: kNumPhases sums and four totals (|Y|, |M|, |H|, S) per sample.
constexpr uint32_t kGatherStatsBytes = 4 * (kNumPhases + 4) * 4;

template <int G, bool STATS>
__global__ __launch_bounds__(1024) void gather_sites_kernel(
    const uint64_t *__restrict__ bits, uint64_t *__restrict__ out,
    const uint32_t *__restrict__ order, uint32_t num_stored, uint32_t words_per_sample,
    GatherStatsArgs st) {
  extern __shared__ uint4 gather_lds[];  // the sites' fields, then a tile per wavefront
  static_assert(G == 2 || G == 4, "a nibble or a byte per site");
  static_assert(kGatherBatch % 8 == 0 && (2 * G * kGatherBatch) % 64 == 0, "whole rounds");
  static_assert(kGatherBatch == 16, "the statistics: 16 lanes per sample");
  const uint32_t P = words_per_sample / 2;
  const uint32_t s0 = blockIdx.x * G;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
  uint8_t *site = reinterpret_cast<uint8_t *>(gather_lds);
  uint8_t *tile = site + ((gather_site_bytes(G, P) + 15u) & ~15u) + wave * kGatherTileBytes;
  // [G][kNumPhases] per-phase sums, then [G][4] totals
  int32_t *phase_sum = reinterpret_cast<int32_t *>(site + ((gather_site_bytes(G, P) + 15u) & ~15u) +
                                                   waves * kGatherTileBytes);
  int32_t *totals = phase_sum + G * kNumPhases;
  if (STATS) {
    for (uint32_t i = threadIdx.x; i < G * (kNumPhases + 4); i += blockDim.x) phase_sum[i] = 0;
    if (blockIdx.x == 0) {
#pragma unroll
      for (uint32_t k = 0; k < kNumCheckShares; ++k)
        if (threadIdx.x == k) st.steps_out[k] = st.steps[k];
    }
  }
  int32_t yc = 0, mc = 0, hc = 0, sa = 0;  // of word lane & 15 of sample lane >> 4, over the batches

  const uint64_t *het[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const uint32_t s = s0 + g < num_stored ? s0 + g : num_stored - 1;  // (repeats: not stored)
    het[g] = bits + (uint64_t)s * words_per_sample;
  }
  for (uint32_t w = threadIdx.x; w < P; w += blockDim.x) {
    uint64_t f[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int g = 0; g < G; ++g) {
      f[gather_field_bit(g, 0)] = het[g][w];
      f[gather_field_bit(g, 1)] = het[g][P + w];
    }
    if (G == 4) {
      uint4 *dst = reinterpret_cast<uint4 *>(site + 64 * w);
#pragma unroll
      for (uint32_t b = 0; b < 8; b += 2) {
        const uint64_t lo = gather_interleave8(f, b), hi = gather_interleave8(f, b + 1);
        dst[b / 2] = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
      }
    } else {
      uint4 *dst = reinterpret_cast<uint4 *>(site + 32 * w);
#pragma unroll
      for (uint32_t b = 0; b < 8; b += 4)
        dst[b / 4] = make_uint4(gather_pack_nibbles(gather_interleave8(f, b)),
                                gather_pack_nibbles(gather_interleave8(f, b + 1)),
                                gather_pack_nibbles(gather_interleave8(f, b + 2)),
                                gather_pack_nibbles(gather_interleave8(f, b + 3)));
    }
  }
  __syncthreads();

  constexpr uint32_t kRounds = kGatherBatch / 8;          // 8 words of 8 bytes: 64 lanes
  constexpr uint32_t kOutRounds = 2 * G * kGatherBatch / 64;
  uint64_t *tile64 = reinterpret_cast<uint64_t *>(tile);
  const uint32_t last_site = 64 * P - 1;
  for (uint32_t w0 = kGatherBatch * wave; w0 < P; w0 += kGatherBatch * waves) {
    uint32_t src[kGatherBatch];
#pragma unroll
    for (uint32_t k = 0; k < kGatherBatch; ++k) {
      const uint32_t W = w0 + k < P ? w0 + k : P - 1;  // (behind the plane: a repeat, not stored)
      const uint32_t at = order[64 * W + lane];
      src[k] = at < last_site ? at : last_site;        // (a permutation: never taken)
    }
    uint32_t field[kGatherBatch];
#pragma unroll
    for (uint32_t k = 0; k < kGatherBatch; ++k) field[k] = site[gather_byte_index(G, src[k])];
#pragma unroll
    for (uint32_t k = 0; k < kGatherBatch; ++k)
      tile[64 * k + lane] = (uint8_t)gather_field_of(G, src[k], field[k]);
    wave_lds_order();
    uint64_t x[kRounds];
#pragma unroll
    for (uint32_t r = 0; r < kRounds; ++r) x[r] = tile64[64 * r + lane];
    wave_lds_order();
#pragma unroll
    for (uint32_t r = 0; r < kRounds; ++r) {
      const uint64_t y = gather_assemble8(x[r]);
      const uint32_t k = 8 * r + (lane >> 3), b = lane & 7;
#pragma unroll
      for (uint32_t f = 0; f < 2 * G; ++f) tile[gather_out_byte(f, k, b)] = (uint8_t)(y >> (8 * f));
    }
    wave_lds_order();
#pragma unroll
    for (uint32_t r = 0; r < kOutRounds; ++r) {
      const uint32_t i = 64 * r + lane, f = gather_out_field(i), k = gather_out_word(i);
      const uint64_t word = tile64[i];
      const uint32_t s = s0 + f / 2;
      if (w0 + k < P && s < num_stored)
        out[(uint64_t)s * words_per_sample + (f & 1) * P + w0 + k] = word;
    }
    if (STATS) {
      // (sample_stats_kernel's expressions, word for word)
      const uint32_t g = (lane >> 4) & (G - 1), w = w0 + (lane & 15);
      const bool in = (lane >> 4) < G && w < P;  // (beyond the plane: contributes nothing)
      const uint64_t h = in ? tile64[gather_field_bit(g, 0) * kGatherBatch + (lane & 15)] : 0ull;
      const uint64_t v = in ? tile64[gather_field_bit(g, 1) * kGatherBatch + (lane & 15)] : 0ull;
      const int32_t y = in ? __popcll(~h) : 0;
      const int32_t m = __popcll(h & v);
      yc += y;
      mc += m;
      hc += __popcll(h & ~v);
      const uint64_t hom_a = in ? ~h & 0xFFFFFFFF00000000ull : 0ull;
      const int32_t t_a = __popcll(hom_a & ~v) - __popcll(hom_a & v);
      sa += t_a;
      // (a k-step is 4 words: 4 neighbouring lanes, the batch starts at a multiple of 16)
      int32_t d = y - m + 2 * t_a;
      d += __shfl_xor(d, 1);
      d += __shfl_xor(d, 2);
      if ((lane & 3) == 0 && in) {
        const uint32_t x = (kNumPhases * ((w >> 2) + 1) - 1) / st.all_steps;
        atomicAdd(&phase_sum[g * kNumPhases + (x < kNumPhases ? x : kNumPhases - 1)], d);
      }
    }
    wave_lds_order();
  }
  // (words_per_sample odd: the word behind the two planes is never read by the conversion)
  if (!STATS) return;
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) {
    yc += __shfl_xor(yc, off);
    mc += __shfl_xor(mc, off);
    hc += __shfl_xor(hc, off);
    sa += __shfl_xor(sa, off);
  }
  if ((lane & 15) == 0 && (lane >> 4) < G) {
    int32_t *t = totals + 4 * (lane >> 4);
    atomicAdd(t, yc);
    atomicAdd(t + 1, mc);
    atomicAdd(t + 2, hc);
    atomicAdd(t + 3, sa);
  }
  __syncthreads();
  const uint32_t ps = s0 + wave;
  if (wave >= G || ps >= num_stored) return;  // whole wavefront
  yc = totals[4 * wave];
  mc = totals[4 * wave + 1];
  hc = totals[4 * wave + 2];
  sa = totals[4 * wave + 3];
  // inclusive scan over the phases -- lane l holds phases 2 l and 2 l + 1 --: the count in
  // front of boundary x + 1 is the scan's value at phase x
  static_assert(kNumPhases == 128, "two phases per lane");
  const int32_t p0 = phase_sum[wave * kNumPhases + 2 * lane];
  const int32_t p1 = phase_sum[wave * kNumPhases + 2 * lane + 1];
  int32_t run = p0 + p1;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int32_t up = __shfl_up(run, off);
    if ((int)lane >= off) run += up;
  }
  // (n_A in front of boundary x: 128 per k-step)
  st.cum[(size_t)(2 * lane) * st.s_stride + ps] =
      (float)(run - p1 + (int32_t)(128u * phase_step(st.all_steps, 2 * lane + 1)));
  if (2 * lane + 1 < kNumCum)
    st.cum[(size_t)(2 * lane + 1) * st.s_stride + ps] =
        (float)(run + (int32_t)(128u * phase_step(st.all_steps, 2 * lane + 2)));
  if (lane == 0) {
    st.stats[ps] = make_float2((float)(yc - mc), (float)hc);
    st.cum[(size_t)kNumCum * st.s_stride + ps] =
        (float)(yc - mc + 2 * sa + (int32_t)(128u * st.all_steps));
    // (the samples sample_stats_kernel's workgroup ps / 4 of stats_grid would have added)
    if (((ps >> 2) & 15) == 0 || st.stats_grid < 64) {
      relaxed_add(st.sums, 1ull);
      relaxed_add(st.sums + 1, (unsigned long long)mc);
      relaxed_add(st.sums + 2, (unsigned long long)hc);
    }
  }
}

// Threads of a gather_sites_kernel<G> workgroup for `P` words per plane: as many wavefronts
// as leave room for their tiles (and the statistics' sums, whether they are taken or not: one
// rule per width) behind the staged sites; 0: the sites do not fit.
uint32_t gather_lds_bytes(int group, uint32_t P, uint32_t threads) {
  return ((gather_site_bytes((uint32_t)group, P) + 15u) & ~15u) + (threads / 64) * kGatherTileBytes +
         kGatherStatsBytes;
}
uint32_t gather_threads(int group, uint32_t P) {
  for (uint32_t threads = 1024; threads >= 512; threads /= 2)
    if (gather_lds_bytes(group, P, threads) <= kGatherLdsMax) return threads;
  return 0;
}

template <int G, bool STATS>
hipError_t launch_gather_form(const uint64_t *d_bit_sets, uint32_t num_stored,
                              uint32_t words_per_sample, const uint32_t *d_order,
                              uint64_t *d_permuted, const GatherStatsArgs &st, hipStream_t stream) {
  const uint32_t P = words_per_sample / 2, threads = gather_threads(G, P);
  if (threads == 0) return hipErrorInvalidValue;
  const hipError_t e = allow_dynamic_lds<gather_sites_kernel<G, STATS>>(kGatherLdsMax);
  if (e != hipSuccess) return e;
  gather_sites_kernel<G, STATS><<<dim3((num_stored + G - 1) / G), dim3(threads),
                                  gather_lds_bytes(G, P, threads), stream>>>(
      d_bit_sets, d_permuted, d_order, num_stored, words_per_sample, st);
  return hipGetLastError();
}

size_t up256(size_t x) { return (x + 255) / 256 * 256; }

// bits of a weight for `n` samples: 6 n^2 / 2 at most
int weight_bits(uint32_t n) {
  int b = 1;
  while (b < 32 && (1ull << b) <= n) ++b;
  return 2 * b + 2 < 64 ? 2 * b + 2 : 64;
}

}  // namespace

SiteOrderScratch site_order_scratch(uint32_t num_stored, uint32_t words_per_sample) {
  SiteOrderScratch l = {};
  const uint32_t P = words_per_sample / 2;
  if (num_stored < 2 || P == 0 || (size_t)P * 16 > kOrderLdsBytes) return l;
  const size_t sites = (size_t)P * 64;
  size_t temp = 0;
  unsigned long long *nil_k = nullptr;
  uint32_t *nil_v = nullptr;
  if (hipcub::DeviceRadixSort::SortPairsDescending(nullptr, temp, nil_k, nil_k, nil_v, nil_v,
                                                   (int)sites, 0, 64) != hipSuccess)
    return l;
  l.counts = 0;                                      // u32 [sites][4]
  l.keys = l.counts + up256(sites * 16);             // u64 in, out; then the phases' sums
  l.vals = l.keys + up256(sites * 16) + up256(kNumPhases * 40);  // u32 in, out
  l.sort_temp = l.vals + up256(sites * 8);
  l.sort_temp_bytes = up256(temp);
  l.permuted = l.sort_temp + l.sort_temp_bytes;
  l.bytes = l.permuted + up256((size_t)num_stored * words_per_sample * 8);
  return l;
}

hipError_t launch_site_order(const uint64_t *d_bit_sets, uint32_t num_stored,
                             uint32_t words_per_sample, const PlaneGeometry &geo, void *d_scratch,
                             const SiteOrderScratch &l, SiteCurve *d_curve, hipStream_t stream) {
  if (l.bytes == 0 || d_scratch == nullptr) return hipErrorInvalidValue;
  const uint32_t P = words_per_sample / 2, sites = P * 64;
  uint8_t *base = static_cast<uint8_t *>(d_scratch);
  uint32_t *counts = reinterpret_cast<uint32_t *>(base + l.counts);
  unsigned long long *keys_in = reinterpret_cast<unsigned long long *>(base + l.keys);
  unsigned long long *keys_out = keys_in + sites;
  unsigned long long *phase_w =
      reinterpret_cast<unsigned long long *>(base + l.keys + up256((size_t)sites * 16));
  double *phase_v = reinterpret_cast<double *>(phase_w + kNumPhases);
  uint32_t *vals_in = reinterpret_cast<uint32_t *>(base + l.vals), *vals_out = vals_in + sites;
  hipError_t e = hipMemsetAsync(counts, 0, (size_t)sites * 16, stream);
  if (e != hipSuccess) return e;
  e = launch_site_counts(d_bit_sets, num_stored, words_per_sample, counts, stream);
  if (e != hipSuccess) return e;
  site_keys_kernel<<<dim3((sites + 255) / 256), dim3(256), 0, stream>>>(counts, sites, keys_in,
                                                                       vals_in);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  size_t temp = l.sort_temp_bytes;
  e = hipcub::DeviceRadixSort::SortPairsDescending(base + l.sort_temp, temp, keys_in, keys_out,
                                                   vals_in, vals_out, (int)sites, 0,
                                                   weight_bits(num_stored), stream);
  if (e != hipSuccess) return e;
  site_curve_kernel<<<dim3(kNumPhases), dim3(256), 0, stream>>>(counts, vals_out, sites,
                                                                geo.k_words / 8, phase_w, phase_v);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  site_curve_scan_kernel<<<dim3(1), dim3(64), 0, stream>>>(phase_w, phase_v, d_curve);
  return hipGetLastError();
}

int site_gather_pick(int option, uint32_t words_per_sample) {
  const uint32_t P = words_per_sample / 2;
  if (P == 0 || (size_t)P * 16 > kOrderLdsBytes) return option <= 0 ? 0 : -1;
  if (option == 0) return 0;
  if ((option == -1 || option == 4) && gather_threads(4, P) != 0) return 4;
  if ((option == -1 || option == 2) && gather_threads(2, P) != 0) return 2;
  return option == -1 ? 0 : -1;
}

hipError_t launch_site_gather(const uint64_t *d_bit_sets, uint32_t num_stored,
                              uint32_t words_per_sample, const uint32_t *d_order,
                              uint64_t *d_permuted, int gather, const SiteGatherStats *fused,
                              hipStream_t stream) {
  const uint32_t P = words_per_sample / 2;
  if (num_stored == 0 || P == 0 || (size_t)P * 16 > kOrderLdsBytes) return hipErrorInvalidValue;
  if (gather == 4 || gather == 2) {
    GatherStatsArgs st = {};
    if (fused != nullptr) {
      const PlaneGeometry &geo = fused->geo;
      // (plane sample = stored sample, and every one of them inside the conversion's range)
      const uint32_t s_end = fused->s_end < geo.s_stride ? fused->s_end : geo.s_stride;
      if (!geo.diag || geo.num_rows != num_stored || s_end < num_stored || geo.k_words < 8)
        return hipErrorInvalidValue;
      st.stats = fused->to.stats;
      st.cum = fused->to.cum;
      st.sums = fused->to.sums;
      st.steps_out = fused->to.steps;
      st.s_stride = geo.s_stride;
      st.all_steps = geo.k_words / 8;
      st.stats_grid = (s_end + 3) / 4;  // (launch_sample_stats over plane samples [0, s_end))
      for (uint32_t k = 0; k < kNumCheckShares; ++k)
        st.steps[k] = check_step_of(st.all_steps, k, filter_check_min_steps());
    }
    if (gather == 4)
      return fused ? launch_gather_form<4, true>(d_bit_sets, num_stored, words_per_sample, d_order,
                                                 d_permuted, st, stream)
                   : launch_gather_form<4, false>(d_bit_sets, num_stored, words_per_sample,
                                                  d_order, d_permuted, st, stream);
    return fused ? launch_gather_form<2, true>(d_bit_sets, num_stored, words_per_sample, d_order,
                                               d_permuted, st, stream)
                 : launch_gather_form<2, false>(d_bit_sets, num_stored, words_per_sample, d_order,
                                                d_permuted, st, stream);
  }
  if (gather != 0 || fused != nullptr) return hipErrorInvalidValue;
  const uint32_t groups2 = (num_stored + 1) / 2;
  if ((size_t)P * 32 <= kOrderLdsBytes)
    permute_sites_kernel<2><<<dim3(groups2), dim3(256), P * 32, stream>>>(
        d_bit_sets, d_permuted, d_order, num_stored, words_per_sample);
  else
    permute_sites_kernel<1><<<dim3(num_stored), dim3(256), P * 16, stream>>>(
        d_bit_sets, d_permuted, d_order, num_stored, words_per_sample);
  return hipGetLastError();
}

hipError_t launch_site_permute(const uint64_t *d_bit_sets, uint32_t num_stored,
                               uint32_t words_per_sample, void *d_scratch,
                               const SiteOrderScratch &l, int gather,
                               const SiteGatherStats *fused, hipStream_t stream) {
  if (l.bytes == 0 || d_scratch == nullptr) return hipErrorInvalidValue;
  const uint32_t sites = (words_per_sample / 2) * 64;
  uint8_t *base = static_cast<uint8_t *>(d_scratch);
  const uint32_t *vals_out = reinterpret_cast<const uint32_t *>(base + l.vals) + sites;
  uint64_t *permuted = reinterpret_cast<uint64_t *>(base + l.permuted);
  return launch_site_gather(d_bit_sets, num_stored, words_per_sample, vals_out, permuted, gather,
                            fused, stream);
}

SiteOrderForecast site_order_forecast(const SiteCurve &c, uint32_t num_stored, uint32_t k_words,
                                      float thr) {
  SiteOrderForecast f = {0, 0, false};
  const float sites = 32.f * (float)k_words, ns = (float)num_stored;
  if (!(ns > 0.f && c.het_calls != 0)) return f;
  // (bound_level() of king_filter.hip)
  const float m = (float)c.missing_calls / (ns * sites), h = (float)c.het_calls / (ns * sites);
  const float mean = m * (1.f + m / (2.f * h * (1.f - m))), sigma = 1.f / sqrtf(sites);
  f.verdict_first = mean - 4.f * sigma > thr;
  const float k_lin = mean + 4.6f * sigma + 0.003f, k_ord = mean + 4.6f * c.sigma + 0.003f;
  if (k_lin < 0.5f) {
    const float f64 = 64.f * (1.f - 2.f * thr) / (1.f - 2.f * k_lin);
    if (f64 <= 62.f) f.stored64 = f64 > 32.f ? (uint32_t)ceilf(f64) : 32u;
  }
  if (k_ord < 0.5f) {
    const float need = (1.f - 2.f * thr) / (1.f - 2.f * k_ord);
    for (uint32_t s = 32; s <= 62 && f.order64 == 0; ++s)
      if (site_curve_covers(c.cum, 0, s, need)) f.order64 = s;
  }
  return f;
}

}  // namespace cuking
