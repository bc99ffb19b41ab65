// Site QC (include/cuking_amd.h, "Site QC"): what the kernels of king_site_qc.hip, their
// launches and the host-side tests share -- the bit-sliced counters of a lane of the count
// kernel, the table a keep mask is turned into once per compaction call, and the function that
// assembles one output word from it.  Plain C++: hipcc compiles the functions for the device,
// the sanitizer build of the tests (tests/site_qc_host_driver.cc) for the host, where they run
// against plain sums and cuking_compact_sites_host.
#ifndef CUKING_AMD_KING_SITE_QC_H_
#define CUKING_AMD_KING_SITE_QC_H_

#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#define CUKING_HD __host__ __device__
#else
#define CUKING_HD
#endif

namespace cuking {

// ---- site counts: the bit-sliced counters of a lane of site_counts_kernel -------------------
constexpr uint32_t kSiteGroup = 8;                       // samples per adder tree
constexpr uint32_t kSiteUpperPlanes = 6;                 // planes of weight 8 .. 256
constexpr uint32_t kSitePlanes = 3 + kSiteUpperPlanes;
// 504: the most a wavefront may count (a multiple of the group, below 2^9 - 1)
constexpr uint32_t kSiteWaveSamples = ((1u << kSitePlanes) - 1) / kSiteGroup * kSiteGroup;

// sum and carry of three bit vectors
CUKING_HD inline void csa(uint64_t a, uint64_t b, uint64_t c, uint64_t &sum, uint64_t &carry) {
  const uint64_t u = a ^ b;
  sum = u ^ c;
  carry = (a & b) | (u & c);
}

// One class's vertical counter: bit b of plane[k] is bit k of the count of site b.
struct SliceCounter {
  uint64_t plane[kSitePlanes];
  CUKING_HD void clear() {
#pragma unroll
    for (uint32_t k = 0; k < kSitePlanes; ++k) plane[k] = 0;
  }
  CUKING_HD void add8(const uint64_t x[kSiteGroup]) {
    uint64_t two_a, two_b, four_a, four_b, eight;
    csa(plane[0], x[0], x[1], plane[0], two_a);
    csa(plane[0], x[2], x[3], plane[0], two_b);
    csa(plane[1], two_a, two_b, plane[1], four_a);
    csa(plane[0], x[4], x[5], plane[0], two_a);
    csa(plane[0], x[6], x[7], plane[0], two_b);
    csa(plane[1], two_a, two_b, plane[1], four_b);
    csa(plane[2], four_a, four_b, plane[2], eight);
#pragma unroll
    for (uint32_t k = 3; k < kSitePlanes; ++k) {  // ripple the carry of weight 8 upwards
      const uint64_t carry = plane[k] & eight;
      plane[k] ^= eight;
      eight = carry;
    }
  }
  // the count of bit `bit` (< 32) of the low or the high half of the planes
  CUKING_HD uint32_t count(uint32_t half, uint32_t bit) const {
    uint32_t v = 0;
#pragma unroll
    for (uint32_t k = 0; k < kSitePlanes; ++k) {
      const uint32_t p = half ? (uint32_t)(plane[k] >> 32) : (uint32_t)plane[k];
      v |= ((p >> bit) & 1u) << k;
    }
    return v;
  }
};

// ---- compaction ----------------------------------------------------------------------------
// One input plane word of a compaction: the move masks of the parallel-suffix compress of
// `keep` (Hacker's Delight 7-4: six steps move every kept bit to the low end, in order),
// the mask itself and the number of kept sites in front of the word.
struct CompactWord {
  uint64_t move[6];
  uint64_t keep;
  uint64_t prefix;
};
static_assert(sizeof(CompactWord) == 64, "one cache line half per input word");

// The table of a call: CompactWord[plane_in], then uint32 first_in[plane_out] -- the input
// word that holds kept site 64 j (plane_in where there is none: the word is all padding).
inline size_t compact_table_bytes(uint32_t plane_in, uint32_t plane_out) {
  return (size_t)plane_in * sizeof(CompactWord) + (size_t)plane_out * sizeof(uint32_t);
}

inline void compact_move_masks(uint64_t m, uint64_t move[6]) {
  uint64_t mk = ~m << 1;  // the bits to the right of which a 0 is counted
  for (int i = 0; i < 6; ++i) {
    uint64_t mp = mk ^ (mk << 1);  // parallel suffix
    mp ^= mp << 2;
    mp ^= mp << 4;
    mp ^= mp << 8;
    mp ^= mp << 16;
    mp ^= mp << 32;
    const uint64_t mv = mp & m;  // the bits that move 2^i places in this step
    move[i] = mv;
    m = (m ^ mv) | (mv >> (1u << i));
    mk &= ~mp;
  }
}

// Fills `table` (compact_table_bytes) from keep[plane_in]; returns the number of kept sites.
inline uint64_t build_compact_table(const uint64_t *keep, uint32_t plane_in, uint32_t plane_out,
                                    void *table) {
  CompactWord *words = static_cast<CompactWord *>(table);
  uint32_t *first_in = reinterpret_cast<uint32_t *>(words + plane_in);
  uint64_t kept = 0;
  uint32_t next = 0;  // the output word whose first site has not been met yet
  for (uint32_t w = 0; w < plane_in; ++w) {
    compact_move_masks(keep[w], words[w].move);
    words[w].keep = keep[w];
    words[w].prefix = kept;
    kept += (uint64_t)__builtin_popcountll(keep[w]);
    // (a run of empty words passes by here: kept does not move)
    while (next < plane_out && (uint64_t)next * 64 < kept) first_in[next++] = w;
  }
  while (next < plane_out) first_in[next++] = plane_in;
  return kept;
}

CUKING_HD inline uint64_t compact_compress(uint64_t x, const CompactWord &e) {
  x &= e.keep;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const uint64_t t = x & e.move[i];
    x = (x ^ t) | (t >> (1u << i));
  }
  return x;
}

// Samples a thread of the kernel serves with one walk over the table.
constexpr uint32_t kCompactRows = 4;

// Output word `j` of both planes for `rows` (<= kCompactRows) samples whose input rows are
// `pitch` words apart: the kept bits of the input words first_in[j] .. that fall into sites
// [64 j, 64 j + 64) of the output, every bit from `kept` on set (missing).
CUKING_HD inline void compact_output_word(const CompactWord *words, const uint32_t *first_in,
                                          uint32_t plane_in, uint64_t kept, const uint64_t *in,
                                          uint64_t pitch, uint32_t rows, uint32_t j,
                                          uint64_t het[kCompactRows], uint64_t hom[kCompactRows]) {
  const uint64_t base = (uint64_t)j * 64;
#pragma unroll
  for (uint32_t r = 0; r < kCompactRows; ++r) het[r] = hom[r] = 0;
  for (uint32_t w = first_in[j]; w < plane_in; ++w) {
    const CompactWord e = words[w];
    if (e.prefix >= base + 64) break;
    if (e.keep == 0) continue;
    // prefix + popcount(keep) > base for the first word, prefix < base + 64 for all: the
    // shift is in (-64, 64)
    const int64_t at = (int64_t)e.prefix - (int64_t)base;
#pragma unroll
    for (uint32_t r = 0; r < kCompactRows; ++r) {
      if (r >= rows) continue;
      const uint64_t a = compact_compress(in[r * pitch + w], e);
      const uint64_t b = compact_compress(in[r * pitch + plane_in + w], e);
      het[r] |= at >= 0 ? a << at : a >> -at;
      hom[r] |= at >= 0 ? b << at : b >> -at;
    }
  }
  const uint64_t pad = kept >= base + 64 ? 0 : kept <= base ? ~0ull : ~0ull << (kept - base);
#pragma unroll
  for (uint32_t r = 0; r < kCompactRows; ++r) {
    het[r] |= pad;
    hom[r] |= pad;
  }
}

}  // namespace cuking

#endif  // CUKING_AMD_KING_SITE_QC_H_
