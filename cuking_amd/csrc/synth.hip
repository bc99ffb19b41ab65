// Device-side synthetic genotype generator for benchmarks and parity runs at
// sizes whose COO Parquet form would be 10^9 .. 10^11 rows.
// The reference has no counterpart.  Specification (integer only, so the CPU
// twins -- oracle/synth_oracle.c for the baseline, tests/synth_models_twin.py for
// every model -- are bit-identical; u32 scale: a probability p is floor(p * 2^32)):
//   mix64      splitmix64 finaliser
//   hash3      mix64(mix64(seed + tag*GOLD + a) ^ (b * 0xD1B54A32D192ED03))
//   founder    two alleles: lo32 / hi32 of hash3(seed,2,founder,site) < AF of the
//              site in the founder's ancestry
//   missing    lo32(hash3(seed,3,sample,site)) < the sample's missing threshold
//   duplicate  its founder's genotype (own missing draw)
//   child      one allele from each founder parent, each parent's genotype drawn in
//              that parent's ancestry; a het parent transmits bit 0 / bit 1 of
//              hash3(seed,4,child,site)
// The cohort models differ in three small tables only:
//   0 baseline  AF = AF_LO + (hi32(hash3(seed,1,site,0)) * AF_SPAN >> 32), i.e.
//               uniform on [0.05, 0.5); one ancestry; every sample misses 1 %
//   1 exome     AF = spectrum(hash3(seed,1,site,0)), log-uniform on [2^-13, 1/2):
//               spectrum(h) = (2^31 | (lo32(h) >> 1)) >> k, k = 1 + (hi32(h) * 12 >> 32)
//               (octave k uniform in 1..12, linear inside the octave); one ancestry; 1 %
//   2 admixed   ancestry of a founder = bit 0 of hash3(seed,5,founder,0);
//               AF in ancestry A = the exome value; in ancestry B the same value
//               unless lo32(hash3(seed,8,site,0)) < 2^30 (one site in four), where it
//               is spectrum(hash3(seed,6,site,0));
//               missing threshold of a sample from h = hash3(seed,7,sample,0):
//               lo32(h) < 1 %: the tail, 10 % + (hi32(h) * 20 % >> 32), otherwise
//               0.5 % + (hi32(h) * 3 % >> 32)  (0.5 % .. 3.5 %, mean 2 %)
// Output: the reference bitset layout (cuking.cu:507-523).
#include <hip/hip_runtime.h>

#include "king_common.h"

namespace cuking {

namespace {

constexpr uint64_t kTagSite = 1, kTagGeno = 2, kTagMiss = 3, kTagTrans = 4, kTagAncestry = 5,
                   kTagSiteB = 6, kTagCallRate = 7, kTagDiverged = 8;
constexpr uint32_t kAfLo = 214748364u;     // floor(0.05 * 2^32)
constexpr uint32_t kAfSpan = 1932735283u;  // floor(0.45 * 2^32)
constexpr uint32_t kMissThr = 42949672u;   // floor(0.01 * 2^32)
constexpr uint32_t kOctaves = 12;
constexpr uint32_t kDivergedThr = 1u << 30;       // one site in four
constexpr uint32_t kTailThr = 42949672u;          // floor(0.01 * 2^32) of the samples
constexpr uint32_t kTailMissLo = 429496729u;      // floor(0.10 * 2^32)
constexpr uint32_t kTailMissSpan = 858993459u;    // floor(0.20 * 2^32)
constexpr uint32_t kMissLo = 21474836u;           // floor(0.005 * 2^32)
constexpr uint32_t kMissSpan = 128849018u;        // floor(0.03 * 2^32)
constexpr uint32_t kKindDup = 1, kKindChild = 2;
// SynthRow::flags
constexpr uint32_t kRowChild = 1, kRowAncestryA = 2, kRowAncestryB = 4;

constexpr const char *kModelNames[kNumSynthModels] = {"baseline", "exome", "admixed"};

__device__ __forceinline__ uint64_t mix64(uint64_t x) {
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

__device__ __forceinline__ uint64_t hash3(uint64_t seed, uint64_t tag,
                                          uint64_t a, uint64_t b) {
  return mix64(mix64(seed + tag * 0x9E3779B97F4A7C15ull + a) ^
               (b * 0xD1B54A32D192ED03ull));
}

__device__ __forceinline__ uint32_t scale(uint32_t u, uint32_t span) {
  return (uint32_t)(((uint64_t)u * span) >> 32);
}

__device__ __forceinline__ uint32_t spectrum(uint64_t h) {
  const uint32_t k = 1 + scale((uint32_t)(h >> 32), kOctaves);
  return (0x80000000u | ((uint32_t)h >> 1)) >> k;
}

__device__ __forceinline__ uint32_t founder_genotype(uint64_t seed,
                                                     uint32_t founder,
                                                     uint32_t site,
                                                     uint32_t af_thr) {
  const uint64_t h = hash3(seed, kTagGeno, founder, site);
  return ((uint32_t)h < af_thr) + ((uint32_t)(h >> 32) < af_thr);
}

__device__ __forceinline__ uint32_t transmit(uint32_t g, uint32_t coin) {
  return g == 1 ? coin : (g >> 1);
}

// What the fill kernel knows of a site: its allele-frequency threshold in either ancestry.
struct SynthSite {
  uint32_t af[2];
};
// ... and of a sample: its missing threshold, the founder(s) its alleles come from (a
// founder: itself; a duplicate: its founder, twice) and kRow* flags.
struct SynthRow {
  uint32_t miss_thr, src_a, src_b, flags;
};

// The two table kernels are the only code that knows the models.
__global__ __launch_bounds__(256) void synth_site_table_kernel(
    const int model, const uint64_t seed, const uint32_t num_sites, const uint32_t table_sites,
    SynthSite *__restrict__ sites) {
  const uint32_t site = blockIdx.x * blockDim.x + threadIdx.x;
  if (site >= table_sites) return;
  SynthSite out = {{0, 0}};  // (padding sites of the last word: never drawn)
  if (site < num_sites) {
    const uint64_t h = hash3(seed, kTagSite, site, 0);
    if (model == kSynthBaseline) {
      out.af[0] = out.af[1] = kAfLo + scale((uint32_t)(h >> 32), kAfSpan);
    } else {
      out.af[0] = out.af[1] = spectrum(h);
      if (model == kSynthAdmixed &&
          (uint32_t)hash3(seed, kTagDiverged, site, 0) < kDivergedThr)
        out.af[1] = spectrum(hash3(seed, kTagSiteB, site, 0));
    }
  }
  sites[site] = out;
}

__global__ __launch_bounds__(256) void synth_row_table_kernel(
    const int model, const uint64_t seed, const uint32_t *__restrict__ kind,
    const uint32_t *__restrict__ pa, const uint32_t *__restrict__ pb,
    const uint32_t sample_begin, const uint32_t sample_end, SynthRow *__restrict__ rows) {
  const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= sample_end - sample_begin) return;
  const uint32_t s = sample_begin + row;
  const uint32_t k = kind[s];
  SynthRow out = {kMissThr, s, s, 0};
  if (k == kKindDup) {
    out.src_a = out.src_b = pa[s];
  } else if (k == kKindChild) {
    out.src_a = pa[s];
    out.src_b = pb[s];
    out.flags = kRowChild;
  }
  if (model == kSynthAdmixed) {
    if (hash3(seed, kTagAncestry, out.src_a, 0) & 1) out.flags |= kRowAncestryA;
    if (hash3(seed, kTagAncestry, out.src_b, 0) & 1) out.flags |= kRowAncestryB;
    const uint64_t h = hash3(seed, kTagCallRate, s, 0);
    const uint32_t u = (uint32_t)(h >> 32);
    out.miss_thr = (uint32_t)h < kTailThr ? kTailMissLo + scale(u, kTailMissSpan)
                                          : kMissLo + scale(u, kMissSpan);
  }
  rows[row] = out;
}

// One wavefront = up to 64 consecutive words of one sample's planes; a lane = one site of
// the word in hand, so the site table is read 512 contiguous bytes at a time, everything
// about the sample is wave-uniform (scalar registers, uniform branches) and a ballot is
// the word.  Lane i keeps word i; one coalesced store per plane at the end.
__global__ __launch_bounds__(256) void synth_fill_kernel(
    const uint64_t seed, const SynthSite *__restrict__ sites, const SynthRow *__restrict__ rows,
    const uint32_t num_rows, const uint32_t sample_begin, const uint32_t num_sites,
    const uint32_t words_per_sample, uint64_t *__restrict__ bit_set, const uint64_t block_offset) {
  const uint32_t plane = words_per_sample / 2;
  const uint32_t chunks = (plane + 63) / 64;
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t wave = (block_offset + blockIdx.x) * (blockDim.x / 64) +
                        __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (wave >= (uint64_t)num_rows * chunks) return;
  const uint32_t row = (uint32_t)(wave / chunks);
  const uint32_t w0 = (uint32_t)(wave % chunks) * 64;
  const uint32_t words = min(64u, plane - w0);
  const SynthRow r = rows[row];
  const uint32_t s = sample_begin + row;
  const bool child = (r.flags & kRowChild) != 0;
  const uint32_t anc_a = (r.flags & kRowAncestryA) ? 1 : 0;
  const uint32_t anc_b = (r.flags & kRowAncestryB) ? 1 : 0;

  uint64_t het_word = 0, hom_word = 0;
  for (uint32_t i = 0; i < words; ++i) {
    const uint32_t site = (w0 + i) * 64 + lane;  // (< 2^32: the table has plane * 64 entries)
    uint32_t g = 3;
    if (site < num_sites && (uint32_t)hash3(seed, kTagMiss, s, site) >= r.miss_thr) {
      const SynthSite t = sites[site];
      g = founder_genotype(seed, r.src_a, site, anc_a ? t.af[1] : t.af[0]);
      if (child) {
        const uint64_t ht = hash3(seed, kTagTrans, s, site);
        g = transmit(g, (uint32_t)(ht & 1)) +
            transmit(founder_genotype(seed, r.src_b, site, anc_b ? t.af[1] : t.af[0]),
                     (uint32_t)((ht >> 1) & 1));
      }
    }
    // (het, hom_var): 0 -> 00, 1 -> 10, 2 -> 01, missing -> 11
    const uint64_t het = __builtin_amdgcn_ballot_w64((g & 1) != 0);
    const uint64_t hom = __builtin_amdgcn_ballot_w64(g >= 2);
    if (lane == i) {
      het_word = het;
      hom_word = hom;
    }
  }
  if (lane < words) {
    uint64_t *dst = bit_set + (uint64_t)row * words_per_sample + w0 + lane;
    dst[0] = het_word;
    dst[plane] = hom_word;
  }
}

// One wavefront that watches the two clocks of its compute unit for a fixed
// wall time: s_memtime ticks with the shader clock, s_memrealtime at a constant
// 100 MHz, so delta / delta x 100 MHz is the clock the chip sustains while
// whatever else is running (MI355X_MICROARCH.md, "DVFS give-back" item 6).  It
// sleeps between looks and leaves after `ticks_100mhz` of real time whatever
// happens.  out = {shader ticks, real ticks}.
__global__ __launch_bounds__(64) void clock_probe_kernel(uint64_t ticks_100mhz,
                                                         uint64_t *out) {
  const uint64_t r0 = __builtin_amdgcn_s_memrealtime();
  const uint64_t c0 = __builtin_amdgcn_s_memtime();
  uint64_t r1 = r0;
  while (r1 - r0 < ticks_100mhz) {
    __builtin_amdgcn_s_sleep(127);
    r1 = __builtin_amdgcn_s_memrealtime();
  }
  const uint64_t c1 = __builtin_amdgcn_s_memtime();
  r1 = __builtin_amdgcn_s_memrealtime();
  if (threadIdx.x == 0) {
    out[0] = c1 - c0;
    out[1] = r1 - r0;
  }
}

}  // namespace

hipError_t launch_clock_probe(uint64_t microseconds, uint64_t *d_out,
                              hipStream_t stream) {
  clock_probe_kernel<<<dim3(1), dim3(64), 0, stream>>>(microseconds * 100, d_out);
  return hipGetLastError();
}

const char *synth_model_name(int model) {
  return model >= 0 && model < kNumSynthModels ? kModelNames[model] : "";
}

size_t synth_table_bytes(uint32_t num_rows, uint32_t words_per_sample) {
  return (size_t)(words_per_sample / 2) * 64 * sizeof(SynthSite) +
         (size_t)num_rows * sizeof(SynthRow);
}

hipError_t launch_synth(int model, uint64_t seed, const uint32_t *d_kind,
                        const uint32_t *d_pa, const uint32_t *d_pb,
                        uint32_t sample_begin, uint32_t sample_end,
                        uint32_t num_sites, uint32_t words_per_sample,
                        void *d_tables, uint64_t *d_bit_set, hipStream_t stream) {
  const uint32_t num_rows = sample_end - sample_begin;
  const uint32_t plane = words_per_sample / 2;
  if (num_rows == 0 || plane == 0) return hipSuccess;
  if (plane > 0xFFFFFFFFu / 64) return hipErrorInvalidValue;  // site indices are u32
  const uint32_t table_sites = plane * 64;
  SynthSite *sites = static_cast<SynthSite *>(d_tables);
  SynthRow *rows = reinterpret_cast<SynthRow *>(sites + table_sites);
  synth_site_table_kernel<<<dim3((table_sites + 255) / 256), dim3(256), 0, stream>>>(
      model, seed, num_sites, table_sites, sites);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  synth_row_table_kernel<<<dim3((num_rows + 255) / 256), dim3(256), 0, stream>>>(
      model, seed, d_kind, d_pa, d_pb, sample_begin, sample_end, rows);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  const uint64_t waves = (uint64_t)num_rows * ((plane + 63) / 64);
  const uint64_t blocks = (waves + 3) / 4;
  const uint64_t cap = 0xFFFFFFFFull / 256;  // < 2^32 threads per launch
  for (uint64_t done = 0; done < blocks; done += cap) {
    const uint64_t n = blocks - done < cap ? blocks - done : cap;
    synth_fill_kernel<<<dim3((uint32_t)n), dim3(256), 0, stream>>>(
        seed, sites, rows, num_rows, sample_begin, num_sites, words_per_sample, d_bit_set, done);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace cuking
