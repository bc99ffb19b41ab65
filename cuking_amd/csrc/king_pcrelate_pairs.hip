// PC-Relate for listed pairs on the device (include/cuking_amd.h "PC-Relate for listed pairs"
// holds the contract, king_pcrelate.h the element functions and the per-site update as code,
// king_host.cc the host twin that runs the very same chains; DESIGN.md 4.3f the reasons for the
// shape): pcrelate_pairs_kernel.
//
// One THREAD owns one pair and walks the sites in ascending order, so each of the seven sums is
// literally the one chain of the definition: no cross-lane reduction, no atomics, no scratch,
// and a row that depends on nothing but its own pair.  The thread holds the X rows of both
// samples in 2 D registers (zero-padded, statically indexed), the smaller index first.
//
// Per step of kPairStep = 64 sites (one word of each plane):
//   stage    the workgroup copies beta[64][D] into LDS, zeros for sites >= num_sites and columns
//            >= d: a zero row gives mu = 0, which no bound admits, so the tail sites are zero
//            operands, not code paths.  One fetch of a beta row serves the kPairThreads = 512
//            pairs of the workgroup.
//   words    the four words of the step (het and hom_var of both samples) were loaded one step
//            ahead; the loads of the next step are issued before the step's arithmetic.
//   sites    per site both mu chains read the beta row as LDS broadcasts, then
//            pcrelate_pair_site.
// The epilogue is pcrelate_pair_result and eight plain dword stores per pair.  A pair with an
// index >= num_stored reads nothing and stores the row of a pair without a jointly valid site.
#include <hip/hip_runtime.h>

#include "king_common.h"
#include "king_device.h"
#include "king_pcrelate.h"

namespace cuking {

namespace {

constexpr uint32_t kPairThreads = 512;  // pairs of a workgroup: one per thread
constexpr uint32_t kPairStep = 64;      // sites per step: one word of each plane
static_assert(sizeof(cuking_pcrelate_pair) == 32, "eight dwords per output row");

struct PcrPairArgs {
  const uint64_t *bits;
  const float *x;
  const float *beta;
  const float *f;
  const unsigned char *pairs;
  cuking_pcrelate_pair *out;
  uint64_t num_pairs;
  uint64_t pair_base;  // first pair of this launch
  uint32_t pair_stride;
  uint32_t num_stored, words_per_sample, num_sites, ldx, ldbeta, d;
  float lo, hi;
};

template <uint32_t D>
__global__ __launch_bounds__(kPairThreads) void pcrelate_pairs_kernel(const PcrPairArgs a) {
  __shared__ __attribute__((aligned(16))) float beta_lds[kPairStep * D];
  const uint32_t tid = threadIdx.x;
  const uint64_t p = a.pair_base + (uint64_t)blockIdx.x * kPairThreads + tid;
  const bool have_pair = p < a.num_pairs;

  // ---- the pair: the input order goes to the output, the smaller index leads the chains
  uint32_t in_i = 0, in_j = 0;
  if (have_pair) {
    const uint32_t *entry = reinterpret_cast<const uint32_t *>(a.pairs + p * a.pair_stride);
    in_i = entry[0];
    in_j = entry[1];
  }
  const bool active = have_pair && in_i < a.num_stored && in_j < a.num_stored;
  const uint32_t si = in_i < in_j ? in_i : in_j, sj = in_i < in_j ? in_j : in_i;
  const uint32_t plane_words = a.words_per_sample / 2;
  const uint64_t *bits_i = a.bits + (uint64_t)(active ? si : 0) * a.words_per_sample;
  const uint64_t *bits_j = a.bits + (uint64_t)(active ? sj : 0) * a.words_per_sample;
  const bool reads = active && a.num_sites != 0;  // (the arrays may be null without sites)

  float xi[D], xj[D];
#pragma unroll
  for (uint32_t c = 0; c < D; ++c) xi[c] = xj[c] = 0.0f;
  float one_plus_f_i = 1.0f, one_plus_f_j = 1.0f;
  if (reads) {
    const float *ri = a.x + (uint64_t)si * a.ldx, *rj = a.x + (uint64_t)sj * a.ldx;
#pragma unroll
    for (uint32_t c = 0; c < D; ++c)
      if (c < a.d) {
        xi[c] = ri[c];
        xj[c] = rj[c];
      }
    if (a.f != nullptr) {
      one_plus_f_i = 1.0f + a.f[si];
      one_plus_f_j = 1.0f + a.f[sj];
    }
  }

  PcrelatePairSums sum;
  const uint32_t steps = (uint32_t)(((uint64_t)a.num_sites + kPairStep - 1) / kPairStep);
  // (w < steps <= plane_words: num_sites <= 64 plane_words; an inactive thread reads as missing)
  uint64_t het_i = ~0ull, hom_i = ~0ull, het_j = ~0ull, hom_j = ~0ull;
  if (reads) {
    het_i = bits_i[0];
    hom_i = bits_i[plane_words];
    het_j = bits_j[0];
    hom_j = bits_j[plane_words];
  }
  for (uint32_t w = 0; w < steps; ++w) {
    const uint64_t s0 = (uint64_t)w * kPairStep;
    // ---- stage beta: loads in flight before the barrier that frees the LDS of the step before
    constexpr uint32_t kItems = (kPairStep * D + kPairThreads - 1) / kPairThreads;
    float bv[kItems];
#pragma unroll
    for (uint32_t i = 0; i < kItems; ++i) {
      const uint32_t idx = i * kPairThreads + tid;
      const uint64_t s = s0 + idx / D;
      const uint32_t c = idx % D;
      bv[i] = (idx < kPairStep * D && s < a.num_sites && c < a.d) ? a.beta[s * a.ldbeta + c] : 0.0f;
    }
    // ---- the words of the next step
    uint64_t next_het_i = ~0ull, next_hom_i = ~0ull, next_het_j = ~0ull, next_hom_j = ~0ull;
    if (reads && w + 1 < steps) {
      next_het_i = bits_i[w + 1];
      next_hom_i = bits_i[plane_words + w + 1];
      next_het_j = bits_j[w + 1];
      next_hom_j = bits_j[plane_words + w + 1];
    }
    __syncthreads();  // (the step before has been read)
#pragma unroll
    for (uint32_t i = 0; i < kItems; ++i) {
      const uint32_t idx = i * kPairThreads + tid;
      if (idx < kPairStep * D) beta_lds[idx] = bv[i];
    }
    __syncthreads();

    // ---- the sites of the step, in ascending order
#pragma unroll 2
    for (uint32_t s = 0; s < kPairStep; ++s) {
      const float *row = beta_lds + s * D;
      const float mu_i = pcrelate_mu(xi, row, D);
      const float mu_j = pcrelate_mu(xj, row, D);
      pcrelate_pair_site(&sum, geno_code(het_i, hom_i, s), mu_i, one_plus_f_i,
                         geno_code(het_j, hom_j, s), mu_j, one_plus_f_j, a.lo, a.hi);
    }
    het_i = next_het_i;
    hom_i = next_hom_i;
    het_j = next_het_j;
    hom_j = next_hom_j;
  }

  if (have_pair) {
    cuking_pcrelate_pair row;
    row.sample_i = in_i;
    row.sample_j = in_j;
    pcrelate_pair_result(sum, &row.kin, &row.k0, &row.k1, &row.k2);
    row.ibs0 = sum.ibs0;
    row.sites = sum.sites;
    a.out[p] = row;
  }
}

}  // namespace

hipError_t launch_pcrelate_pairs(const uint64_t *d_bits, uint32_t num_stored,
                                 uint32_t words_per_sample, uint32_t num_sites, const float *d_x,
                                 uint32_t ldx, const float *d_beta, uint32_t ldbeta, uint32_t d,
                                 float lo, float hi, const float *d_f, const void *d_pairs,
                                 uint64_t num_pairs, uint32_t pair_stride,
                                 cuking_pcrelate_pair *d_out, hipStream_t stream) {
  if (num_pairs == 0) return hipSuccess;
  PcrPairArgs a;
  a.bits = d_bits;
  a.x = d_x;
  a.beta = d_beta;
  a.f = d_f;
  a.pairs = static_cast<const unsigned char *>(d_pairs);
  a.out = d_out;
  a.num_pairs = num_pairs;
  a.pair_base = 0;
  a.pair_stride = pair_stride;
  a.num_stored = num_stored;
  a.words_per_sample = words_per_sample;
  a.num_sites = num_sites;
  a.ldx = ldx;
  a.ldbeta = ldbeta;
  a.d = d;
  a.lo = lo;
  a.hi = hi;
  const uint64_t blocks = (num_pairs + kPairThreads - 1) / kPairThreads;
  return pcrelate_dispatch_columns(d, [&](auto columns) {
    return launch_in_chunks(blocks, kPairThreads, [&](uint64_t done, uint32_t n) {
      a.pair_base = done * kPairThreads;
      pcrelate_pairs_kernel<decltype(columns)::value>
          <<<dim3(n), dim3(kPairThreads), 0, stream>>>(a);
    });
  });
}

}  // namespace cuking
