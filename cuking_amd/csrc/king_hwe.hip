// Hardy-Weinberg exact test per site on the device (include/cuking_amd.h "Hardy-Weinberg test"
// holds the contract, king_hwe.h the walk as code, king_host.cc the host twin that calls the same
// function site by site; DESIGN.md 4.3l the reasons for the shape): hwe_sites_kernel.
//
// One THREAD owns one site: it loads the site's 16-byte count row (one dwordx4 per lane, 1 KiB
// contiguous per wavefront), walks hwe_exact_p -- one chain of dependent fp64 multiplies and
// divides, in the one order the contract names -- and stores the p-value.  No LDS, no atomics, no
// scratch, nothing data-dependent that can fail.  A workgroup is ONE wavefront: the trip count of
// a site is its rare homozygote count plus half its heterozygote count, orders of magnitude apart
// between a rare and a common site, and a wavefront that is done frees its slot for the next
// instead of waiting for three others.
#include <hip/hip_runtime.h>

#include "king_common.h"
#include "king_device.h"
#include "king_hwe.h"

namespace cuking {

namespace {

constexpr uint32_t kHweThreads = 64;  // one wavefront
static_assert(kHweMidp == CUKING_HWE_MIDP, "one flag");

__global__ __launch_bounds__(kHweThreads) void hwe_sites_kernel(const uint4 *counts,
                                                                uint32_t num_sites, uint32_t midp,
                                                                double *p, uint64_t block_base) {
  const uint64_t s = (block_base + blockIdx.x) * kHweThreads + threadIdx.x;
  if (s >= num_sites) return;
  const uint4 c = counts[s];  // hom_ref, het, hom_var, missing (ignored)
  p[s] = hwe_exact_p(c.x, c.y, c.z, midp != 0);
}

}  // namespace

hipError_t launch_hwe_sites(const uint32_t *d_counts, uint32_t num_sites, bool midp, double *d_p,
                            hipStream_t stream) {
  const uint64_t blocks = ((uint64_t)num_sites + kHweThreads - 1) / kHweThreads;
  return launch_in_chunks(blocks, kHweThreads, [&](uint64_t done, uint32_t n) {
    hwe_sites_kernel<<<dim3(n), dim3(kHweThreads), 0, stream>>>(
        reinterpret_cast<const uint4 *>(d_counts), num_sites, midp ? 1u : 0u, d_p, done);
  });
}

}  // namespace cuking
