// Unrelated set and families from the records (cuking_unrelated_set, cuking_unrelated_set_host):
// the definitions the device kernels (king_prune.hip), the host implementation (king_host.cc)
// and the tests share, so that they cannot drift apart.  Plain C++ without a HIP header;
// usable from host and device.
//
// Edge.  A record (cuking_result) is an EDGE between sample_i and sample_j when
// `kin > prune_threshold` -- the strict float32 comparison a record itself makes
// (unrel_is_edge).  A NaN prune_threshold is refused; -inf makes every record with a kinship
// above -inf an edge (a record never carries less: it passed `kin > kin_threshold` itself).
// Records may repeat -- a pair may appear more than once, e.g. in the concatenated buffers of
// several shards --; repeats count once.  EVERY record, edge or not, must satisfy sample_i <
// sample_j < num_samples (unrel_record_valid): one that does not makes the call fail with
// CUKING_ERR_INVALID_ARGUMENT, and nothing is read or written outside the per-sample arrays
// because of it (such a record never becomes an edge).
//
// Priority key.  One uint64 per sample, unrel_key(priority[s], s): for a number it is
// kin_best_key(priority[s], s) of king_kin_summary.h -- the order-preserving map of the
// float32 priority in the high word, ~s in the low word -- so that under unsigned comparison
// the higher priority wins and, among equals, the LOWER sample index.  A NaN priority is taken
// as lower than every number: high word 0 (-inf maps to 0x007FFFFF), low word ~s as for any
// other sample.  No two samples share a key, and no key is 0 (s < 2^31).
//
// Default priority.  When the caller gives none: -(float)degree[s], degree = the number of
// DISTINCT partners of s among the edges (fewer relatives first; exact below 2^24 partners).
//
// Unrelated set.  The samples taken in descending key order: a sample is KEPT (keep byte 1)
// if none of its neighbours was kept before it, else DROPPED (keep byte 0) -- the
// lexicographically first maximal independent set of that order.  A sample without edges is
// kept.  The result is a function of the edge SET and the keys alone.  This is NOT Hail's
// maximal_independent_set, which removes the currently highest-degree vertex and recomputes
// the degrees: that has no parallel form with a unique answer.
//
// Family.  family[s] = the lowest sample index of the connected component of s in the edge
// graph; s itself for a sample without edges.
//
// Limits of the device call (32-bit index arithmetic): num_samples at most 2^31, num_records
// at most 2^30.
#ifndef CUKING_AMD_KING_UNRELATED_H_
#define CUKING_AMD_KING_UNRELATED_H_

#include <stddef.h>
#include <stdint.h>

#include "king_kin_summary.h"

namespace cuking {

constexpr uint8_t kUnrelDropped = 0, kUnrelKept = 1;
// (only while the device rounds run; never in a result)
constexpr uint8_t kUnrelUndecided = 2;
constexpr uint32_t kUnrelMaxSamples = 0x80000000u, kUnrelMaxRecords = 0x40000000u;

CUKING_SUMMARY_HD inline bool unrel_threshold_valid(float prune_threshold) {
  return prune_threshold == prune_threshold;
}
CUKING_SUMMARY_HD inline bool unrel_is_edge(float kin, float prune_threshold) {
  return kin > prune_threshold;
}
CUKING_SUMMARY_HD inline bool unrel_record_valid(uint32_t sample_i, uint32_t sample_j,
                                                 uint32_t num_samples) {
  return sample_i < sample_j && sample_j < num_samples;
}
// The key of sample s (file header): THE definition.
CUKING_SUMMARY_HD inline uint64_t unrel_key(float priority, uint32_t s) {
  if (priority != priority) return (uint64_t)(uint32_t)~s;
  return kin_best_key(priority, s);
}
CUKING_SUMMARY_HD inline float unrel_default_priority(uint32_t degree) { return -(float)degree; }
// An edge as one word, i in the high half: what the duplicate removal compares.
CUKING_SUMMARY_HD inline uint64_t unrel_edge_word(uint32_t i, uint32_t j) {
  return ((uint64_t)i << 32) | j;
}

// ---- the device half (king_prune.hip), called by cuking_unrelated_set (king_abi.hip) ------
// Workspace of one call, in bytes: control words, 20 B per sample (key, proposal, degree),
// two edge lists of 8 B per record (the rounds ping-pong between them) and, for the default
// priority only, the table the duplicate removal hashes the edges into (8 B x the power of
// two from twice the records on).
size_t prune_workspace_bytes(uint32_t num_records, uint32_t num_samples, bool default_priority);
// Enqueues the whole computation on `stream` (a hipStream_t) and WAITS for it between the
// batches of rounds.  Returns 0, or the hipError_t of a failing runtime call; *invalid = 1
// for a record that is not valid (the outputs are then unspecified), *exceeded = 1 if a loop
// ran past its bound (an internal error).
int prune_run(void *workspace, const cuking_result *d_records, uint32_t num_records,
              uint32_t num_samples, float prune_threshold, const float *d_priority,
              uint8_t *d_keep, uint32_t *d_family, uint32_t num_cus, uint32_t *rounds,
              uint32_t *host_syncs, int *invalid, int *exceeded, void *stream);

}  // namespace cuking

#endif  // CUKING_AMD_KING_UNRELATED_H_
