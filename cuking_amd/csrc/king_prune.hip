// Unrelated set and families from the records, on the device (cuking_unrelated_set): the
// device half of the contract in king_unrelated.h.  The records stay where cuking_compute_king
// appended them; what leaves the GPU is one byte and one word per sample.
//
// Steps, all on the caller's stream:
//   init     per sample: undecided, no proposal, degree 0, label = own index.
//   build    one pass over the records: validity (a flag word), the threshold test, and a
//            wavefront-aggregated append of (i, j) to edge list A -- one atomic per wavefront,
//            as the record kernels reserve their slots.  Repeats stay in the list: the rounds
//            and the families are idempotent in them.  For the default priority each edge
//            word also goes into an open-addressing table (linear probing from a mixed hash,
//            load at most 1/2); the lane whose compare-and-swap claims the slot counts the
//            edge at both ends' degrees, a lane that finds its own word there does not.
//   keys     per sample, from the priority or the degree.
//   families on list A: hook (atomicMin of the smaller root label into the larger root) and
//            compress (pointer jumping to the root), until a hook pass changes nothing.
//            Labels only ever decrease and always name a sample of the same component, so
//            the fixed point -- one root per component, the lowest index -- does not depend
//            on the order of the atomics.
//   rounds   until no live edge is left.  Round r reads list r & 1 and writes the other:
//              propose  a live edge with both ends undecided raises each end's proposal word
//                       to the other end's key (64-bit atomicMax) and is appended to the other
//                       list; an edge with a decided end dies here;
//              decide   an undecided sample whose key beats its proposal is KEPT; proposals
//                       go back to 0, the round is counted if it had a live edge;
//              mark     a surviving edge with a KEPT end marks the other end DROPPED (many
//                       lanes may store the same byte).
//            The undecided sample with the largest key is kept in every round, so there are at
//            most num_samples rounds; a round on an empty list keeps every sample still
//            undecided and changes nothing else.  (Compaction sits in `propose` rather than
//            behind `mark` so that the count of live edges, and with it `rounds`, is a function
//            of the graph: an edge is live in round r iff both its ends are undecided when the
//            round starts, whatever `mark` of the round before raced with.)
// The host reads three words back per BATCH of rounds (kRoundBatch) and one per batch of
// family passes: the call waits for the stream, like the record count it follows.
//
// Every loop is a grid-stride loop over a grid sized from the CU count; indices are 32-bit
// (num_samples <= 2^31, num_records <= 2^30); all stores are plain C++ stores or HIP atomics.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "king_unrelated.h"

namespace cuking {

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kBlocksPerCu = 4;
// Rounds enqueued between two reads of the live count (how it was chosen;
// env CUKING_AMD_PRUNE_BATCH overrides it for that measurement), and family passes between
// two reads of the changed flag.
constexpr uint32_t kRoundBatch = 4;
constexpr uint32_t kFamilyBatch = 2;

// Control words (uint32) at the front of the workspace.
enum : uint32_t {
  kCtlInvalid = 0,   // a record that is not valid was seen
  kCtlLive = 1,      // [2]: entries of edge list A / B
  kCtlRounds = 3,    // rounds that had a live edge
  kCtlChanged = 4,   // [kFamilyBatch]: the hook pass changed a label
  kCtlTableFull = 6, // the duplicate table had no free slot (cannot happen at load 1/2)
  kCtlWords = 64
};
constexpr uint64_t kEmptySlot = ~0ull;  // (no edge word: i < j < 2^31)

size_t align256(size_t x) { return (x + 255) / 256 * 256; }

uint32_t table_slots(uint32_t num_records) {
  uint32_t slots = 1024;
  while (slots < 2ull * num_records) slots <<= 1;  // (num_records <= 2^30: at most 2^31)
  return slots;
}

struct Layout {
  size_t key, nbr, degree, label, list_a, list_b, table, bytes;
  uint32_t slots;
};
Layout layout(uint32_t num_records, uint32_t num_samples, bool default_priority) {
  Layout l;
  size_t at = align256(kCtlWords * sizeof(uint32_t));
  l.key = at, at += align256((size_t)num_samples * 8);
  l.nbr = at, at += align256((size_t)num_samples * 8);
  l.degree = at, at += align256((size_t)num_samples * 4);
  l.label = at, at += align256((size_t)num_samples * 4);
  l.list_a = at, at += align256((size_t)num_records * 8);
  l.list_b = at, at += align256((size_t)num_records * 8);
  l.slots = default_priority ? table_slots(num_records) : 0;
  l.table = at, at += align256((size_t)l.slots * 8);
  l.bytes = at;
  return l;
}

__device__ inline uint32_t grid_first() { return blockIdx.x * blockDim.x + threadIdx.x; }
__device__ inline uint32_t grid_stride() { return gridDim.x * blockDim.x; }

// Slot of this lane's entry behind *counter: one atomic per wavefront.  Called by every lane
// of the wavefront (pred false: no entry, the return value is not used).
__device__ inline uint32_t wave_append(uint32_t *counter, bool pred) {
  const uint64_t mask = __ballot(pred);
  if (mask == 0) return 0;
  const uint32_t lane = threadIdx.x & 63u;
  const int leader = __ffsll((unsigned long long)mask) - 1;
  uint32_t base = 0;
  if ((int)lane == leader) base = atomicAdd(counter, (uint32_t)__popcll(mask));
  base = __shfl(base, leader);
  return base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
}

__device__ inline uint64_t mix64(uint64_t x) {
  x ^= x >> 33;
  x *= 0xFF51AFD7ED558CCDull;
  x ^= x >> 33;
  x *= 0xC4CEB9FE1A85EC53ull;
  x ^= x >> 33;
  return x;
}

__global__ void prune_init_kernel(uint32_t num_samples, uint8_t *__restrict__ state,
                                  unsigned long long *__restrict__ nbr,
                                  uint32_t *__restrict__ degree, uint32_t *__restrict__ label) {
  for (uint32_t s = grid_first(); s < num_samples; s += grid_stride()) {
    state[s] = kUnrelUndecided;
    nbr[s] = 0;
    degree[s] = 0;
    label[s] = s;
  }
}

// Records -> edge list A (ctl[kCtlLive]); with a table, the distinct-partner degrees too.
// (`first` runs over wavefront-aligned indices below 2^30 + stride: no 32-bit overflow; every
//  lane of a wavefront makes the same number of trips, which wave_append needs.)
__global__ void prune_build_kernel(const cuking_result *__restrict__ records, uint32_t num_records,
                                   uint32_t num_samples, float prune_threshold,
                                   uint32_t *__restrict__ ctl, uint2 *__restrict__ list_a,
                                   unsigned long long *__restrict__ table, uint32_t slots,
                                   uint32_t *__restrict__ degree) {
  const uint32_t lane = threadIdx.x & 63u;
  for (uint32_t first = grid_first() - lane; first < num_records; first += grid_stride()) {
    const uint32_t r = first + lane;
    bool edge = false;
    uint32_t i = 0, j = 0;
    if (r < num_records) {
      i = records[r].sample_i;
      j = records[r].sample_j;
      if (!unrel_record_valid(i, j, num_samples)) {
        ctl[kCtlInvalid] = 1;  // (never an edge: nothing is indexed by i or j)
      } else {
        edge = unrel_is_edge(records[r].kin, prune_threshold);
      }
    }
    const uint32_t slot = wave_append(&ctl[kCtlLive], edge);
    if (!edge) continue;
    list_a[slot] = make_uint2(i, j);  // (slot < num_records: one per record at most)
    if (slots == 0) continue;
    const unsigned long long word = unrel_edge_word(i, j);
    uint32_t at = (uint32_t)mix64(word) & (slots - 1);
    bool placed = false;
    for (uint32_t probe = 0; probe < slots; ++probe, at = (at + 1) & (slots - 1)) {
      const unsigned long long seen = atomicCAS(&table[at], kEmptySlot, word);
      if (seen == kEmptySlot) {  // first of its kind
        atomicAdd(&degree[i], 1u);
        atomicAdd(&degree[j], 1u);
        placed = true;
        break;
      }
      if (seen == word) {  // a repeat
        placed = true;
        break;
      }
    }
    if (!placed) ctl[kCtlTableFull] = 1;
  }
}

__global__ void prune_keys_kernel(uint32_t num_samples, const float *__restrict__ priority,
                                  const uint32_t *__restrict__ degree,
                                  unsigned long long *__restrict__ key) {
  for (uint32_t s = grid_first(); s < num_samples; s += grid_stride())
    key[s] = unrel_key(priority != nullptr ? priority[s] : unrel_default_priority(degree[s]), s);
}

// ---- families ------------------------------------------------------------------------------
__global__ void family_hook_kernel(const uint2 *__restrict__ edges, const uint32_t *__restrict__ count,
                                   uint32_t *__restrict__ label, uint32_t *__restrict__ changed) {
  const uint32_t n = *count;
  for (uint32_t e = grid_first(); e < n; e += grid_stride()) {
    const uint2 ij = edges[e];
    // (a label may be lowered by another lane meanwhile: any value read names a sample of the
    //  same component that is no larger than an earlier one)
    const uint32_t a = __hip_atomic_load(&label[ij.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t b = __hip_atomic_load(&label[ij.y], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (a == b) continue;
    atomicMin(&label[a > b ? a : b], a > b ? b : a);
    *changed = 1;
  }
}

// label[s] = the root of s.  Roots (label[r] == r) do not move during this kernel; every chain
// descends strictly, so it ends at one.
__global__ void family_compress_kernel(uint32_t num_samples, uint32_t *__restrict__ label) {
  for (uint32_t s = grid_first(); s < num_samples; s += grid_stride()) {
    uint32_t l = __hip_atomic_load(&label[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (;;) {
      const uint32_t up = __hip_atomic_load(&label[l], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (up >= l) break;  // (== l: a root; > l cannot happen)
      l = up;
    }
    __hip_atomic_store(&label[s], l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ void family_copy_kernel(uint32_t num_samples, const uint32_t *__restrict__ label,
                                   uint32_t *__restrict__ family) {
  for (uint32_t s = grid_first(); s < num_samples; s += grid_stride()) family[s] = label[s];
}

// ---- rounds --------------------------------------------------------------------------------
// Live edges of `in` (ctl[live_in] entries) with both ends undecided propose and move to `out`
// (ctl[live_out], zero when the kernel starts).
__global__ void round_propose_kernel(const uint2 *__restrict__ in, uint2 *__restrict__ out,
                                     uint32_t *__restrict__ ctl, uint32_t live_in, uint32_t live_out,
                                     const uint8_t *__restrict__ state,
                                     const unsigned long long *__restrict__ key,
                                     unsigned long long *__restrict__ nbr) {
  const uint32_t n = ctl[live_in];
  const uint32_t lane = threadIdx.x & 63u;
  for (uint32_t first = grid_first() - lane; first < n; first += grid_stride()) {
    const uint32_t e = first + lane;
    bool live = false;
    uint2 ij = make_uint2(0, 0);
    if (e < n) {
      ij = in[e];
      live = state[ij.x] == kUnrelUndecided && state[ij.y] == kUnrelUndecided;
    }
    const uint32_t slot = wave_append(&ctl[live_out], live);
    if (!live) continue;
    out[slot] = ij;  // (slot < n: at most one per entry read)
    atomicMax(&nbr[ij.x], key[ij.y]);
    atomicMax(&nbr[ij.y], key[ij.x]);
  }
}

__global__ void round_decide_kernel(uint32_t num_samples, uint32_t *__restrict__ ctl,
                                    uint32_t live_in, uint32_t live_out,
                                    uint8_t *__restrict__ state,
                                    const unsigned long long *__restrict__ key,
                                    unsigned long long *__restrict__ nbr) {
  if (grid_first() == 0) {
    if (ctl[live_out] != 0) ctl[kCtlRounds] += 1;
    ctl[live_in] = 0;  // the next round appends here; this round has read it
  }
  for (uint32_t s = grid_first(); s < num_samples; s += grid_stride()) {
    if (state[s] != kUnrelUndecided) continue;
    if (key[s] > nbr[s]) state[s] = kUnrelKept;
    nbr[s] = 0;
  }
}

__global__ void round_mark_kernel(const uint2 *__restrict__ edges, const uint32_t *__restrict__ ctl,
                                  uint32_t live, uint8_t *__restrict__ state) {
  const uint32_t n = ctl[live];
  for (uint32_t e = grid_first(); e < n; e += grid_stride()) {
    const uint2 ij = edges[e];
    // (only `decide` writes KEPT, and never at both ends of an edge)
    const uint8_t si = state[ij.x], sj = state[ij.y];
    if (si == kUnrelKept) state[ij.y] = kUnrelDropped;
    if (sj == kUnrelKept) state[ij.x] = kUnrelDropped;
  }
}

uint32_t grid_for(uint64_t work, uint32_t num_cus) {
  const uint64_t blocks = (work + kThreads - 1) / kThreads;
  const uint64_t cap = (uint64_t)(num_cus ? num_cus : 1) * kBlocksPerCu;
  return (uint32_t)(blocks < 1 ? 1 : (blocks < cap ? blocks : cap));
}

uint32_t round_batch() {
  if (const char *v = getenv("CUKING_AMD_PRUNE_BATCH")) {
    const int k = atoi(v);
    if (k >= 1 && k <= 1024) return (uint32_t)k;
  }
  return kRoundBatch;
}

}  // namespace

size_t prune_workspace_bytes(uint32_t num_records, uint32_t num_samples, bool default_priority) {
  return layout(num_records, num_samples, default_priority).bytes;
}

#define PRUNE_TRY(expr)                     \
  do {                                      \
    const hipError_t _e = (expr);           \
    if (_e != hipSuccess) return (int)_e;   \
  } while (0)

int prune_run(void *workspace, const cuking_result *d_records, uint32_t num_records,
              uint32_t num_samples, float prune_threshold, const float *d_priority,
              uint8_t *d_keep, uint32_t *d_family, uint32_t num_cus, uint32_t *rounds,
              uint32_t *host_syncs, int *invalid, int *exceeded, void *stream_handle) {
  hipStream_t stream = (hipStream_t)stream_handle;
  const bool default_priority = d_priority == nullptr;
  const Layout l = layout(num_records, num_samples, default_priority);
  uint8_t *base = static_cast<uint8_t *>(workspace);
  uint32_t *ctl = reinterpret_cast<uint32_t *>(base);
  auto *key = reinterpret_cast<unsigned long long *>(base + l.key);
  auto *nbr = reinterpret_cast<unsigned long long *>(base + l.nbr);
  auto *degree = reinterpret_cast<uint32_t *>(base + l.degree);
  auto *label = reinterpret_cast<uint32_t *>(base + l.label);
  uint2 *lists[2] = {reinterpret_cast<uint2 *>(base + l.list_a),
                     reinterpret_cast<uint2 *>(base + l.list_b)};
  auto *table = reinterpret_cast<unsigned long long *>(base + l.table);
  *rounds = 0;
  *invalid = *exceeded = 0;

  const uint32_t sample_grid = grid_for(num_samples, num_cus);
  const uint32_t edge_grid = grid_for(num_records, num_cus);
  PRUNE_TRY(hipMemsetAsync(ctl, 0, kCtlWords * sizeof(uint32_t), stream));
  if (l.slots != 0) PRUNE_TRY(hipMemsetAsync(table, 0xFF, (size_t)l.slots * 8, stream));
  prune_init_kernel<<<sample_grid, kThreads, 0, stream>>>(num_samples, d_keep, nbr, degree, label);
  prune_build_kernel<<<edge_grid, kThreads, 0, stream>>>(d_records, num_records, num_samples,
                                                         prune_threshold, ctl, lists[0], table,
                                                         l.slots, degree);
  prune_keys_kernel<<<sample_grid, kThreads, 0, stream>>>(num_samples, d_priority, degree, key);
  PRUNE_TRY(hipGetLastError());

  uint32_t words[kCtlWords];
  auto read_control = [&]() -> hipError_t {
    hipError_t e = hipMemcpyAsync(words, ctl, sizeof(words), hipMemcpyDeviceToHost, stream);
    if (e != hipSuccess) return e;
    ++*host_syncs;
    return hipStreamSynchronize(stream);
  };

  // Families first: the rounds overwrite list A from their second round on.
  if (d_family != nullptr) {
    for (uint64_t passes = 0;; passes += kFamilyBatch) {
      if (passes > (uint64_t)num_samples + kFamilyBatch) {  // every changing pass removes a root
        *exceeded = 1;
        return 0;
      }
      PRUNE_TRY(hipMemsetAsync(ctl + kCtlChanged, 0, kFamilyBatch * sizeof(uint32_t), stream));
      for (uint32_t k = 0; k < kFamilyBatch; ++k) {
        family_hook_kernel<<<edge_grid, kThreads, 0, stream>>>(lists[0], ctl + kCtlLive, label,
                                                               ctl + kCtlChanged + k);
        family_compress_kernel<<<sample_grid, kThreads, 0, stream>>>(num_samples, label);
      }
      PRUNE_TRY(hipGetLastError());
      PRUNE_TRY(read_control());
      if (words[kCtlInvalid] != 0) {
        *invalid = 1;
        return 0;
      }
      if (words[kCtlChanged + kFamilyBatch - 1] == 0) break;
    }
    family_copy_kernel<<<sample_grid, kThreads, 0, stream>>>(num_samples, label, d_family);
    PRUNE_TRY(hipGetLastError());
  }

  const uint32_t batch = round_batch();
  for (uint64_t r = 0;;) {
    if (r > num_samples) {  // at most num_samples rounds have a live edge, plus the empty one
      *exceeded = 1;
      return 0;
    }
    for (uint32_t k = 0; k < batch; ++k, ++r) {
      const uint32_t in = (uint32_t)(r & 1), out = in ^ 1u;
      round_propose_kernel<<<edge_grid, kThreads, 0, stream>>>(
          lists[in], lists[out], ctl, kCtlLive + in, kCtlLive + out, d_keep, key, nbr);
      round_decide_kernel<<<sample_grid, kThreads, 0, stream>>>(
          num_samples, ctl, kCtlLive + in, kCtlLive + out, d_keep, key, nbr);
      round_mark_kernel<<<edge_grid, kThreads, 0, stream>>>(lists[out], ctl, kCtlLive + out, d_keep);
    }
    PRUNE_TRY(hipGetLastError());
    PRUNE_TRY(read_control());
    if (words[kCtlInvalid] != 0) {
      *invalid = 1;
      return 0;
    }
    if (words[kCtlTableFull] != 0) {
      *exceeded = 1;
      return 0;
    }
    if (words[kCtlLive + (uint32_t)(r & 1)] == 0) break;  // what the last round left alive
  }
  *rounds = words[kCtlRounds];
  return 0;
}

}  // namespace cuking
