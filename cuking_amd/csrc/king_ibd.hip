// IBD segments for listed pairs on the device (include/cuking_amd.h "IBD segments for listed
// pairs" holds the contract, king_ibd.h the word masks and the segment test as code,
// king_host.cc the host twin that walks the same words one by one; DESIGN.md 4.3h the reasons
// for the shape): ibd_group_bits_kernel and ibd_pairs_kernel; and, at the end, the same scan of
// one sample against itself, roh_samples_kernel ("Runs of homozygosity").
//
// One WAVEFRONT owns one pair.  Per step of kIbdStepWords = 64 words (4096 sites) lane l loads
// word 64 step + l of the four planes of the pair (coalesced: 512 bytes per plane and step) and
// of the per-call group-start bitmask; a word without a site below num_sites is not loaded.
// Then, for each kind (king_ibd.h has the masks):
//   edge     bit 63 of the left neighbour's `in` mask, one cross-lane move; lane 0 takes the
//            value carried from the step before
//   scan     every lane offers the last start bit of its word, or "inherit"; an inclusive
//            wavefront scan with the operator "right operand unless it says inherit" (six
//            cross-lane moves), shifted by one lane and seeded with the carried value, tells
//            each lane the first site of the run that is open at its word's entry
//   close    a lane whose word is entered inside a run and has a close bit owns that run: it
//            reads pos[a] and pos[b], makes THE segment test and adds to its own integer
//            counters; with a segment list it takes a slot with one atomic add
//   carry    lane 63's scan value and edge bit go to the next step
// At the end six integer wave reductions (sums and maxima: the order does not matter) feed one
// 40-byte row per pair.  No floating point, no LDS, no scratch.  A pair with an index >=
// num_stored loads nothing and stores zeros.
//
// Bridged breaks (bridge_sites != 0) are a second instantiation of the same kernel, so that
// bridge_sites == 0 launches the code above as it stands.  There the lanes that would make the
// segment test hold a closed run each, in site order along the lanes, and
//   link     a ballot names the lanes with a run; each finds the lane of the run in front of it
//            in the mask, fetches that run with two cross-lane reads -- the first run of a step
//            takes the chain carried from the steps before -- and decides ibd_linked
//   chain    a second ballot names the linked runs; a chain starts at the nearest run at or
//            below the lane that is not linked, its first site is one more cross-lane read, its
//            links a population count of the mask
//   test     a run that is NOT linked ends the chain in front of it: that lane fetches the
//            chain's first site and links, makes THE segment test and takes the list slot
//   carry    the chain of the last run of the step goes to the next step; the word of bit
//            num_sites closes every run, so one test after the loop ends the scan
#include <hip/hip_runtime.h>

#include <type_traits>

#include "king_common.h"
#include "king_device.h"
#include "king_ibd.h"

namespace cuking {

namespace {

constexpr uint32_t kIbdWaves = 4;       // pairs of a workgroup: one per wavefront
constexpr uint32_t kIbdThreads = 64 * kIbdWaves;
constexpr uint32_t kIbdStepWords = 64;  // words per step: one per lane
static_assert(sizeof(cuking_ibd_pair) == 40, "ten dwords per output row");
static_assert(sizeof(cuking_ibd_segment) == 16, "four dwords per segment");

// One thread per bit of the mask, one wavefront per word: the ballot IS the word.
__global__ __launch_bounds__(kIbdThreads) void ibd_group_bits_kernel(
    const int32_t *__restrict__ group, uint32_t num_sites, uint64_t *__restrict__ group_bits) {
  const uint64_t s = (uint64_t)blockIdx.x * kIbdThreads + threadIdx.x;
  const uint64_t word = __ballot(s <= num_sites && ibd_group_start(group, num_sites, s));
  // (whole wavefronts: s / 64 is the same for all 64 lanes)
  if ((threadIdx.x & 63) == 0 && s / 64 < ibd_scan_words(num_sites)) group_bits[s / 64] = word;
}

struct IbdArgs {
  const uint64_t *bits;
  const uint64_t *group_bits;
  const uint32_t *pos;  // or nullptr: pos[s] = s
  const unsigned char *pairs;
  cuking_ibd_pair *out;
  cuking_ibd_segment *segments;
  unsigned long long *count;  // or nullptr: segments are not enumerated
  uint64_t max_segments;
  uint64_t num_pairs;
  uint64_t pair_base;  // first pair of this launch
  uint32_t pair_stride;
  uint32_t num_stored, words_per_sample, num_sites, min_sites, min_length;
};
// ... and what the bridging instantiation reads on top
struct IbdBridgeArgs : IbdArgs {
  uint32_t *bridged;  // [num_pairs][2] or nullptr
  uint32_t bridge_sites;
};
template <bool kBridge>
using IbdArgsOf = typename std::conditional<kBridge, IbdBridgeArgs, IbdArgs>::type;

// What a wavefront carries from step to step for one kind (the same in every lane), and the
// lane's own sums.
struct IbdKind {
  uint32_t open = kIbdInherit;  // first site of the run open at the end of the step before
  uint32_t edge = 0;            // bit 63 of the last `in` word of the step before
  IbdKindSums sums;
  IbdChain chain;               // bridging only: the chain of the last run so far
};

// Inclusive scan over the lanes with "right operand unless it says inherit".
__device__ __forceinline__ uint32_t ibd_wave_scan(uint32_t v, uint32_t lane) {
#pragma unroll
  for (uint32_t off = 1; off < 64; off <<= 1) {
    const uint32_t left = __shfl_up(v, off);
    if (lane >= off && v == kIbdInherit) v = left;
  }
  return v;
}

// THE segment test of a run or chain [first, end] with `links` bridged breaks, by one lane.
__device__ __forceinline__ void ibd_test(const IbdArgs &a, uint32_t kind, uint64_t p,
                                         uint32_t first, uint32_t end, uint32_t links,
                                         IbdKindSums &sums) {
  const uint32_t pos_a = a.pos != nullptr ? a.pos[first] : first;
  const uint32_t pos_b = a.pos != nullptr ? a.pos[end] : end;
  if (ibd_is_segment(first, end, pos_a, pos_b, a.min_sites, a.min_length)) {
    sums.add(pos_b - pos_a);
    sums.bridged += links;
    if (a.count != nullptr) {
      const unsigned long long slot = atomicAdd(a.count, 1ull);
      if (slot < a.max_segments) {
        cuking_ibd_segment seg;
        seg.pair = (uint32_t)p;
        seg.kind = kind;
        seg.first_site = first;
        seg.last_site = end;
        a.segments[slot] = seg;
      }
    }
  }
}

// The highest lane of a non-empty mask.
__device__ __forceinline__ uint32_t ibd_top_lane(uint64_t mask) {
  return 63 - (uint32_t)__builtin_clzll(mask);
}

// The runs that close in this step, linked into chains (all 64 lanes call this together).
// `event`: the lane holds the closed run [first, end]; the lanes hold them in site order.
__device__ __forceinline__ void ibd_chain_step(const IbdBridgeArgs &a, uint32_t kind, uint64_t p,
                                               uint32_t lane, bool event, uint32_t first,
                                               uint32_t end, IbdKind &k) {
  const uint64_t events = __ballot(event);
  if (events == 0) return;  // (the whole wavefront)
  const IbdChain carried = k.chain;
  const uint64_t below = (1ull << lane) - 1, upto = below | 1ull << lane;
  // link: the run in front of mine is the one of lane q, or the last of the carried chain
  const uint64_t before = events & below;
  const bool inside = before != 0;
  const uint32_t q = inside ? ibd_top_lane(before) : 0;
  uint32_t q_first = __shfl(first, q), q_end = __shfl(end, q);
  if (!inside) {
    q_first = carried.last_first;
    q_end = carried.last_end;
  }
  const bool follows = inside || carried.have != 0;
  const bool linked = event && follows &&
                      ibd_linked(q_first, q_end, first, end, a.bridge_sites, a.group_bits);
  // chain: from the nearest run at or below me that is not linked, or the carried chain
  const uint64_t heads = events & ~__ballot(linked);
  const uint64_t mine = heads & upto;
  const uint32_t h = mine != 0 ? ibd_top_lane(mine) : 0;
  uint32_t chain_first = __shfl(first, h);
  // (the events in (h, lane] are all linked; 2 << 63 is 0: nothing above lane 63)
  uint32_t chain_links = (uint32_t)__builtin_popcountll(events & upto & ~((2ull << h) - 1));
  if (mine == 0) {
    chain_first = carried.first;
    chain_links = carried.links + (uint32_t)__builtin_popcountll(events & upto);
  }
  // test: a run that is not linked ends the chain in front of it
  uint32_t done_first = __shfl(chain_first, q), done_links = __shfl(chain_links, q);
  if (!inside) {
    done_first = carried.first;
    done_links = carried.links;
  }
  if (event && !linked && follows) ibd_test(a, kind, p, done_first, q_end, done_links, k.sums);
  // carry: the chain of the step's last run
  const uint32_t z = ibd_top_lane(events);
  k.chain.have = 1;
  k.chain.first = __shfl(chain_first, z);
  k.chain.links = __shfl(chain_links, z);
  k.chain.last_first = __shfl(first, z);
  k.chain.last_end = __shfl(end, z);
}

// One step of one kind: `in` and `group` are the lane's word w.
template <bool kBridge>
__device__ __forceinline__ void ibd_kind_step(const IbdArgsOf<kBridge> &a, uint32_t kind,
                                              uint64_t p, uint64_t w, uint32_t lane, uint64_t in,
                                              uint64_t group, IbdKind &k) {
  const uint32_t last = (uint32_t)(in >> 63);
  uint32_t prev = __shfl_up(last, 1);
  if (lane == 0) prev = k.edge;
  const uint64_t starts = ibd_starts(in, prev, group), closes = ibd_closes(in, prev, group);
  const uint32_t scan = ibd_wave_scan(ibd_open_start(starts, w), lane);
  uint32_t open = __shfl_up(scan, 1);
  if (lane == 0 || open == kIbdInherit) open = k.open;
  // (prev != 0: site 64 w - 1 is inside a run, so a start precedes this word and `open` is
  //  a site; the run's last site is below num_sites)
  const bool event = prev != 0 && closes != 0;
  if constexpr (kBridge) {
    ibd_chain_step(a, kind, p, lane, event, open, event ? ibd_close_last(closes, w) : 0, k);
  } else {
    if (event) ibd_test(a, kind, p, open, ibd_close_last(closes, w), 0, k.sums);
  }
  const uint32_t tail = __shfl(scan, 63);
  if (tail != kIbdInherit) k.open = tail;
  k.edge = __shfl(last, 63);
}

// (ibd_wave_sum, ibd_wave_max and ibd_wave_sum64 live in king_device.h: king_mendel.hip uses them
//  too)

template <bool kBridge>
__global__ __launch_bounds__(kIbdThreads) void ibd_pairs_kernel(const IbdArgsOf<kBridge> a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t p = a.pair_base + (uint64_t)blockIdx.x * kIbdWaves + threadIdx.x / 64;
  if (p >= a.num_pairs) return;  // (the whole wavefront: there is no barrier below)

  const uint32_t *entry = reinterpret_cast<const uint32_t *>(a.pairs + p * a.pair_stride);
  const uint32_t in_i = entry[0], in_j = entry[1];
  const bool active = in_i < a.num_stored && in_j < a.num_stored;
  const uint32_t plane_words = a.words_per_sample / 2;
  const uint64_t *bits_i = a.bits + (uint64_t)(active ? in_i : 0) * a.words_per_sample;
  const uint64_t *bits_j = a.bits + (uint64_t)(active ? in_j : 0) * a.words_per_sample;

  IbdKind kind1, kind2;
  const uint64_t words = ibd_scan_words(a.num_sites);
  if (active) {
    for (uint64_t w0 = 0; w0 < words; w0 += kIbdStepWords) {
      const uint64_t w = w0 + lane;
      const uint64_t valid = ibd_valid_mask(a.num_sites, w);
      // (valid != 0 implies w < plane_words: num_sites <= 64 plane_words; the last step may be
      //  partial and the word of bit num_sites may lie beyond the plane: neither is loaded)
      uint64_t het_i = 0, hom_i = 0, het_j = 0, hom_j = 0;
      if (valid != 0) {
        het_i = bits_i[w];
        hom_i = bits_i[plane_words + w];
        het_j = bits_j[w];
        hom_j = bits_j[plane_words + w];
      }
      const uint64_t group = w < words ? a.group_bits[w] : 0;
      ibd_kind_step<kBridge>(a, 1, p, w, lane, valid & ~ibd_opp(het_i, hom_i, het_j, hom_j),
                             group, kind1);
      ibd_kind_step<kBridge>(a, 2, p, w, lane, valid & ~ibd_diff(het_i, hom_i, het_j, hom_j),
                             group, kind2);
    }
    if constexpr (kBridge) {
      // (every run is closed by now: the chains that are left are whole)
      if (lane == 0 && kind1.chain.have)
        ibd_test(a, 1, p, kind1.chain.first, kind1.chain.last_end, kind1.chain.links, kind1.sums);
      if (lane == 0 && kind2.chain.have)
        ibd_test(a, 2, p, kind2.chain.first, kind2.chain.last_end, kind2.chain.links, kind2.sums);
    }
  }

  cuking_ibd_pair row;
  row.sample_i = in_i;
  row.sample_j = in_j;
  row.segments1 = ibd_wave_sum(kind1.sums.segments);
  row.segments2 = ibd_wave_sum(kind2.sums.segments);
  row.length1 = ibd_wave_sum64(kind1.sums.length);
  row.length2 = ibd_wave_sum64(kind2.sums.length);
  row.longest1 = ibd_wave_max(kind1.sums.longest);
  row.longest2 = ibd_wave_max(kind2.sums.longest);
  if (lane == 0) a.out[p] = row;
  if constexpr (kBridge) {
    const uint32_t bridged1 = ibd_wave_sum(kind1.sums.bridged);
    const uint32_t bridged2 = ibd_wave_sum(kind2.sums.bridged);
    if (lane == 0 && a.bridged != nullptr) {
      a.bridged[2 * p] = bridged1;
      a.bridged[2 * p + 1] = bridged2;
    }
  }
}

// ---- runs of homozygosity (the header's "Runs of homozygosity") ----------------------------------
// The scan above of a sample with itself: ONE kind, whose break mask is roh_break of the sample's
// two planes, and one wavefront per listed sample.  The arguments are those of the pair kernel
// with `pairs` the list of samples (uint32 each, or nullptr: row r is sample r), num_pairs its
// length and `out` / `bridged` unused: the 24-byte row carries the bridged count itself.
static_assert(sizeof(cuking_roh_sample) == 24, "six dwords per output row");
template <bool kBridge>
struct RohArgs : IbdArgsOf<kBridge> {
  cuking_roh_sample *rows;
};

template <bool kBridge>
__global__ __launch_bounds__(kIbdThreads) void roh_samples_kernel(const RohArgs<kBridge> a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t r = a.pair_base + (uint64_t)blockIdx.x * kIbdWaves + threadIdx.x / 64;
  if (r >= a.num_pairs) return;  // (the whole wavefront: there is no barrier below)

  const uint64_t sample =
      a.pairs != nullptr ? reinterpret_cast<const uint32_t *>(a.pairs)[r] : r;
  const bool active = sample < a.num_stored;
  const uint32_t plane_words = a.words_per_sample / 2;
  const uint64_t *bits = a.bits + (active ? sample : 0) * a.words_per_sample;

  IbdKind k;
  const uint64_t words = ibd_scan_words(a.num_sites);
  if (active) {
    for (uint64_t w0 = 0; w0 < words; w0 += kIbdStepWords) {
      const uint64_t w = w0 + lane;
      const uint64_t valid = ibd_valid_mask(a.num_sites, w);
      // (valid != 0 implies w < plane_words, as in ibd_pairs_kernel)
      uint64_t het = 0, hom = 0;
      if (valid != 0) {
        het = bits[w];
        hom = bits[plane_words + w];
      }
      const uint64_t group = w < words ? a.group_bits[w] : 0;
      ibd_kind_step<kBridge>(a, CUKING_ROH_KIND, r, w, lane, valid & ~roh_break(het, hom), group,
                             k);
    }
    if constexpr (kBridge) {
      // (every run is closed by now: the chain that is left is whole)
      if (lane == 0 && k.chain.have)
        ibd_test(a, CUKING_ROH_KIND, r, k.chain.first, k.chain.last_end, k.chain.links, k.sums);
    }
  }

  cuking_roh_sample row;
  row.length = ibd_wave_sum64(k.sums.length);
  row.sample = (uint32_t)sample;
  row.segments = ibd_wave_sum(k.sums.segments);
  row.longest = ibd_wave_max(k.sums.longest);
  row.bridged = 0;
  if constexpr (kBridge) row.bridged = ibd_wave_sum(k.sums.bridged);
  if (lane == 0) a.rows[r] = row;
}

// What both launches below fill alike; `out` and `bridged` are the pair call's own.
IbdBridgeArgs ibd_common_args(const uint64_t *d_bits, uint32_t num_stored,
                              uint32_t words_per_sample, uint32_t num_sites,
                              const uint64_t *d_group_bits, const uint32_t *d_pos,
                              uint32_t min_sites, uint32_t min_length, uint32_t bridge_sites,
                              const void *d_list, uint64_t num_entries, uint32_t stride,
                              cuking_ibd_segment *d_segments, uint64_t max_segments,
                              unsigned long long *d_count) {
  IbdBridgeArgs a;
  a.bits = d_bits;
  a.group_bits = d_group_bits;
  a.pos = d_pos;
  a.pairs = static_cast<const unsigned char *>(d_list);
  a.out = nullptr;
  a.segments = d_segments;
  a.count = d_count;
  a.max_segments = max_segments;
  a.num_pairs = num_entries;
  a.pair_base = 0;
  a.pair_stride = stride;
  a.num_stored = num_stored;
  a.words_per_sample = words_per_sample;
  a.num_sites = num_sites;
  a.min_sites = min_sites;
  a.min_length = min_length;
  a.bridged = nullptr;
  a.bridge_sites = bridge_sites;
  return a;
}

// One wavefront per entry of the list, in launches of at most the grid limit.  `a` is a copy of
// the kernel's own argument type (not deduced: the strict kernels take the slice they read).
template <class Args>
hipError_t ibd_launch_waves(void (*kernel)(Args), typename std::common_type<Args>::type a,
                            hipStream_t stream) {
  const uint64_t blocks = (a.num_pairs + kIbdWaves - 1) / kIbdWaves;
  return launch_in_chunks(blocks, kIbdThreads, [&](uint64_t done, uint32_t n) {
    a.pair_base = done * kIbdWaves;
    kernel<<<dim3(n), dim3(kIbdThreads), 0, stream>>>(a);
  });
}

}  // namespace

hipError_t launch_ibd_group_bits(const int32_t *d_group, uint32_t num_sites,
                                 uint64_t *d_group_bits, hipStream_t stream) {
  // (at most 2^26 + 1 words: 2^24 + 1 workgroups, below every launch limit)
  const uint64_t blocks = (ibd_scan_words(num_sites) + kIbdWaves - 1) / kIbdWaves;
  ibd_group_bits_kernel<<<dim3((uint32_t)blocks), dim3(kIbdThreads), 0, stream>>>(
      d_group, num_sites, d_group_bits);
  return hipGetLastError();
}

hipError_t launch_ibd_pairs(const uint64_t *d_bits, uint32_t num_stored,
                            uint32_t words_per_sample, uint32_t num_sites,
                            const uint64_t *d_group_bits, const uint32_t *d_pos,
                            uint32_t min_sites, uint32_t min_length, uint32_t bridge_sites,
                            const void *d_pairs, uint64_t num_pairs, uint32_t pair_stride,
                            cuking_ibd_pair *d_out, uint32_t *d_bridged,
                            cuking_ibd_segment *d_segments, uint64_t max_segments,
                            unsigned long long *d_count, hipStream_t stream) {
  if (num_pairs == 0) return hipSuccess;
  IbdBridgeArgs a = ibd_common_args(d_bits, num_stored, words_per_sample, num_sites, d_group_bits,
                                    d_pos, min_sites, min_length, bridge_sites, d_pairs,
                                    num_pairs, pair_stride, d_segments, max_segments, d_count);
  a.out = d_out;
  a.bridged = d_bridged;
  if (bridge_sites == 0) {
    // nothing is linked: the strict kernel (it drops the bridge fields), and no pair has a
    // bridged break
    if (d_bridged != nullptr) {
      const hipError_t err = hipMemsetAsync(d_bridged, 0, num_pairs * 2 * sizeof(uint32_t), stream);
      if (err != hipSuccess) return err;
    }
    return ibd_launch_waves(ibd_pairs_kernel<false>, a, stream);
  }
  return ibd_launch_waves(ibd_pairs_kernel<true>, a, stream);
}

namespace {

template <bool kBridge>
hipError_t launch_roh(const IbdBridgeArgs &from, cuking_roh_sample *d_out, hipStream_t stream) {
  RohArgs<kBridge> a;
  static_cast<IbdArgsOf<kBridge> &>(a) = from;  // (the strict form drops the bridge fields)
  a.rows = d_out;
  return ibd_launch_waves(roh_samples_kernel<kBridge>, a, stream);
}

}  // namespace

hipError_t launch_roh_samples(const uint64_t *d_bits, uint32_t num_stored,
                              uint32_t words_per_sample, uint32_t num_sites,
                              const uint64_t *d_group_bits, const uint32_t *d_pos,
                              uint32_t min_sites, uint32_t min_length, uint32_t bridge_sites,
                              const uint32_t *d_samples, uint64_t num_samples,
                              cuking_roh_sample *d_out, cuking_ibd_segment *d_segments,
                              uint64_t max_segments, unsigned long long *d_count,
                              hipStream_t stream) {
  if (num_samples == 0) return hipSuccess;
  const IbdBridgeArgs a = ibd_common_args(
      d_bits, num_stored, words_per_sample, num_sites, d_group_bits, d_pos, min_sites, min_length,
      bridge_sites, d_samples, num_samples, sizeof(uint32_t), d_segments, max_segments, d_count);
  // (bridge_sites == 0 links nothing: the strict instantiation)
  return bridge_sites == 0 ? launch_roh<false>(a, d_out, stream)
                           : launch_roh<true>(a, d_out, stream);
}

}  // namespace cuking
