// IBD segments for listed pairs (include/cuking_amd.h, "IBD segments for listed pairs"): the
// definitions the kernels of king_ibd.hip, the scan of a block of king_ibd_scan.hip ("IBD scan of
// a block"), the host twins of king_host.cc and the tests share, so that they cannot drift apart:
// the word masks, the walk over the words of one kind (IbdWalk), the chain of bridged runs
// (IbdChain) and the segment test.  Plain C++: hipcc compiles the functions for the device, the
// sanitizer build of the tests (tests/ibd_host_driver.cc) for the host.  Integers only.
//
// Words.  Word w of a plane holds the sites 64 w .. 64 w + 63, site s at bit s & 63.  A scan
// looks at ibd_scan_words(num_sites) = num_sites / 64 + 1 words: the last one holds bit
// num_sites, where the last run closes; it lies beyond the plane when num_sites is a multiple
// of 64, and a word at or beyond the plane is never loaded (its `in` mask is zero anyway).
//
// Per word and kind, with `brk` the break mask (ibd_opp for kind 1, ibd_diff for kind 2, and
// roh_break for the runs of homozygosity of one sample, which are scanned the same way):
//     in     = ibd_valid_mask(num_sites, w) & ~brk     the sites that are inside some run
//     group  bit s set iff site s is the first of its group; bit 0 of word 0 and the bit at
//            num_sites are set, the bits beyond it clear (ibd_group_word)
//     before = in << 1 | prev, prev = bit 63 of the word before's `in` (0 for word 0)
//     starts = in & (~before | group)       bit a: a run starts at site a
//     closes = before & (~in | group)       bit t: the run that holds site t - 1 ends there
// A group boundary inside a run gives a close and a start at the same bit, the close first.
// Along the sites starts and closes alternate, so inside a word:
//   - the run that is open at the word's entry (prev == 1) closes at the word's first close
//     bit, if it has one: b = 64 w + ctz(closes) - 1;
//   - the run that is open at the word's end started at the word's last start bit, if it has
//     one -- otherwise it is the run that was open at the entry ("inherit").
// A run that starts AND closes inside one word has at most 63 sites (bits 0 .. 62, closed at
// bit 63), and a run of 64 or more sites always closes in a later word than it starts in: with
// min_sites >= kIbdMinSites = 64 only the first rule can yield a segment, at most one per word
// and kind, and nobody enumerates bits.  IbdWalk::step is these two rules for whoever takes the
// words one by one (the host twins; ibd_scan_word of king_ibd_scan.hip still restates them, see
// DESIGN.md 4.3j); a wavefront takes 64 words at once (ibd_kind_step of king_ibd.hip).
//
// Bridged breaks ("IBD segments with bridged breaks" in the header).  With bridge_sites != 0 two
// consecutive runs on either side of ONE break site are linked when both have at least
// bridge_sites >= kIbdMinSites sites and no group starts at the break or behind it (ibd_linked),
// and a segment is a maximal chain of linked runs.  Both runs of a link cross a word edge, so
// they are among the runs the first rule yields, in site order; a run that opens and closes
// inside one word lies between its neighbours and keeps them more than one site apart.  IbdChain
// is the chain whose last run is the last one seen: the host twin carries it from word to word
// (IbdChain::step, IbdChain::flush), a wavefront from step to step.
#ifndef CUKING_AMD_KING_IBD_H_
#define CUKING_AMD_KING_IBD_H_

#include <cstddef>
#include <cstdint>

#ifndef CUKING_HD
#ifdef __HIPCC__
#define CUKING_HD __host__ __device__
#else
#define CUKING_HD
#endif
#endif

namespace cuking {

constexpr uint32_t kIbdMinSites = 64;
// "no start in this word": the open run is the one that was open before
constexpr uint32_t kIbdInherit = 0xFFFFFFFFu;

CUKING_HD inline uint64_t ibd_scan_words(uint32_t num_sites) {
  return (uint64_t)num_sites / 64 + 1;
}

// The sites of word w below num_sites.
CUKING_HD inline uint64_t ibd_valid_mask(uint32_t num_sites, uint64_t w) {
  const uint64_t first = w * 64;
  if (first >= num_sites) return 0;
  const uint64_t left = num_sites - first;
  return left >= 64 ? ~0ull : (1ull << left) - 1;
}

// Codes (0, 2) or (2, 0): one sample hom-ref, the other hom-var.
CUKING_HD inline uint64_t ibd_opp(uint64_t het_i, uint64_t hom_i, uint64_t het_j,
                                  uint64_t hom_j) {
  const uint64_t ref_i = ~(het_i | hom_i), var_i = hom_i & ~het_i;
  const uint64_t ref_j = ~(het_j | hom_j), var_j = hom_j & ~het_j;
  return (ref_i & var_j) | (var_i & ref_j);
}

// A site that either sample misses (both bits).
CUKING_HD inline uint64_t ibd_missing(uint64_t het_i, uint64_t hom_i, uint64_t het_j,
                                      uint64_t hom_j) {
  return (het_i & hom_i) | (het_j & hom_j);
}

// Both called and the codes differ.
CUKING_HD inline uint64_t ibd_diff(uint64_t het_i, uint64_t hom_i, uint64_t het_j,
                                   uint64_t hom_j) {
  return ((het_i ^ het_j) | (hom_i ^ hom_j)) & ~ibd_missing(het_i, hom_i, het_j, hom_j);
}

// Runs of homozygosity (the header's "Runs of homozygosity"): the break mask of ONE sample, a
// heterozygous call (code 1).  Missing (both bits) is no break.
CUKING_HD inline uint64_t roh_break(uint64_t het, uint64_t hom) { return het & ~hom; }

CUKING_HD inline uint64_t ibd_starts(uint64_t in, uint64_t prev, uint64_t group) {
  return in & (~(in << 1 | prev) | group);
}
CUKING_HD inline uint64_t ibd_closes(uint64_t in, uint64_t prev, uint64_t group) {
  return (in << 1 | prev) & (~in | group);
}

// The first site of the run that is open at the end of a word with these starts, or
// kIbdInherit.  (A start is a site below num_sites <= 2^32 - 1: never the sentinel.)
CUKING_HD inline uint32_t ibd_open_start(uint64_t starts, uint64_t w) {
  return starts != 0 ? (uint32_t)(w * 64 + 63 - (uint32_t)__builtin_clzll(starts)) : kIbdInherit;
}
// The last site of the run that closes at the first close bit of the word (closes != 0, and
// not bit 0 of word 0: prev is 0 there).
CUKING_HD inline uint32_t ibd_close_last(uint64_t closes, uint64_t w) {
  return (uint32_t)(w * 64 + (uint32_t)__builtin_ctzll(closes) - 1);
}

// Whether site s is the first of its group (s <= num_sites; group may be null: one group).
CUKING_HD inline bool ibd_group_start(const int32_t *group, uint32_t num_sites, uint64_t s) {
  if (s == 0 || s == num_sites) return true;
  return s < num_sites && group != nullptr && group[s] != group[s - 1];
}

// THE segment test of a run [a, b] with pos_a = pos[a], pos_b = pos[b] (pos[s] = s without
// positions; pos_b >= pos_a inside a group).  The length of the segment is pos_b - pos_a.
CUKING_HD inline bool ibd_is_segment(uint32_t a, uint32_t b, uint32_t pos_a, uint32_t pos_b,
                                     uint32_t min_sites, uint32_t min_length) {
  return b - a + 1 >= min_sites && pos_b - pos_a >= min_length;
}
// Its first half alone, for a caller that wants to know whether pos[a] and pos[b] are worth
// reading: false means ibd_is_segment is false whatever the positions.
CUKING_HD inline bool ibd_enough_sites(uint32_t a, uint32_t b, uint32_t min_sites) {
  return b - a + 1 >= min_sites;
}

// Whether the run [a2, b2] is linked to the run [a, b] in front of it.  a2 == b + 2 leaves exactly
// site b + 1 between them, which belongs to no run and lies below num_sites: a break.  group_bits
// is the group-start mask of the call (only read when everything else holds; a2 < num_sites keeps
// both bits inside its ibd_scan_words words).
CUKING_HD inline bool ibd_linked(uint32_t a, uint32_t b, uint32_t a2, uint32_t b2,
                                 uint32_t bridge_sites, const uint64_t *group_bits) {
  if (bridge_sites == 0 || (uint64_t)b + 2 != a2) return false;
  if (b - a + 1 < bridge_sites || b2 - a2 + 1 < bridge_sites) return false;
  const uint64_t brk = (uint64_t)b + 1;
  return ((group_bits[brk >> 6] >> (brk & 63)) & 1) == 0 &&
         ((group_bits[a2 >> 6] >> (a2 & 63)) & 1) == 0;
}

// The chain that ends with the last run seen so far: sites first .. last_end, its last run
// last_first .. last_end, `links` bridged breaks inside.
struct IbdChain {
  uint32_t have = 0, first = 0, last_first = 0, last_end = 0, links = 0;

  // The next closed run [a, b], in site order.  True: the chain [*first_out, *end_out] with
  // *links_out bridged breaks is finished and wants THE segment test.  bridge_sites == 0 links
  // nothing: every run is reported where it closes and nothing is kept for flush().
  CUKING_HD bool step(uint32_t a, uint32_t b, uint32_t bridge_sites, const uint64_t *group_bits,
                      uint32_t *first_out, uint32_t *end_out, uint32_t *links_out) {
    if (bridge_sites == 0) {
      *first_out = a;
      *end_out = b;
      *links_out = 0;
      return true;
    }
    bool done = false;
    if (have && ibd_linked(last_first, last_end, a, b, bridge_sites, group_bits)) {
      ++links;
    } else {
      done = flush(first_out, end_out, links_out);
      have = 1;
      first = a;
      links = 0;
    }
    last_first = a;
    last_end = b;
    return done;
  }
  // After the walk every run is closed: the chain that is left, if any, is whole.
  CUKING_HD bool flush(uint32_t *first_out, uint32_t *end_out, uint32_t *links_out) const {
    if (!have) return false;
    *first_out = first;
    *end_out = last_end;
    *links_out = links;
    return true;
  }
};

// The walk over the words of one kind, one word at a time in ascending w.
struct IbdWalk {
  uint32_t prev = 0;            // bit 63 of the word before's `in`
  uint32_t open = kIbdInherit;  // first site of the run that is open at the end of that word

  // Word w with its `in` and group masks.  True: the run [*a, *b] that was open at the word's
  // entry closes in it.
  CUKING_HD bool step(uint64_t in, uint64_t group, uint64_t w, uint32_t *a, uint32_t *b) {
    const uint64_t starts = ibd_starts(in, prev, group), closes = ibd_closes(in, prev, group);
    const bool closed = prev != 0 && closes != 0;
    if (closed) {
      *a = open;
      *b = ibd_close_last(closes, w);
    }
    const uint32_t start = ibd_open_start(starts, w);
    if (start != kIbdInherit) open = start;
    prev = (uint32_t)(in >> 63);
    return closed;
  }
};

// What a pair accumulates per kind; the sums and maxima are integers, so the order in which
// the segments arrive does not matter.
struct IbdKindSums {
  uint32_t segments = 0, longest = 0;
  uint64_t length = 0;
  uint32_t bridged = 0;  // links inside the counted segments
  CUKING_HD void add(uint32_t len) {
    ++segments;
    length += len;
    longest = len > longest ? len : longest;
  }
};

}  // namespace cuking

#endif  // CUKING_AMD_KING_IBD_H_
