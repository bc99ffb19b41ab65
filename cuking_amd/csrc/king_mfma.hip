// The KING pair kernel on the gfx950 matrix cores.
//
// popcount(x & y) over the sites of two bit planes is the dot product of the
// two 0/1 vectors, so the four sums kinship needs (cuking.cu:232-239) are five
// plane products per pair:
//     opp = A_i.R_j + R_i.A_j      bh = H_i.H_j
//     hi  = H_i.D_j                hj = D_i.H_j
// (A hom-alt, R hom-ref, H het, D defined; the full form adds
// hom_hom = (A|R)_i.(A|R)_j).  v_mfma_scale_f32_32x32x64_f8f6f4 with fp4 (E2M1)
// operands does 32 x 32 pairs x 64 sites per instruction in 32 cycles, four
// times the bf16 rate; products and sums are small integers, exact in the
// float32 accumulators while every sum stays below 2^24 (kMfmaMaxSites).
//
// Operand expansion costs ONE VALU instruction per dword.  A lane's fragment
// is 32 fp4 values = 4 dwords.  From four 32-site words of the reference's two
// planes (het, hom_var) one v_bitop3_b32 per dword computes e.g.
// ~het & hom_var & (0x11111111 << f): site 4q+f of each word lands in nibble q
// as the fp4 code 1 << f, i.e. the value 2^(f-1) (0.5, 1, 2).  Both operands
// carry the same factor, and the instruction's E8M0 block scale (2^(1-f) on
// each side) takes it out again, so every product is exactly 1.0 (f = 1 needs
// no scale and uses the unscaled instruction).  f = 3 would be the sign bit:
// those sites are shifted down to position 0 first.  The order of the sites
// inside the k dimension is irrelevant as long as both operands agree.
//
// Workgroup = 128 x 128 pairs, 4 wavefronts (one per SIMD, up to 512
// registers each), each 64 x 64 pairs = 2 x 2 MFMA blocks x 4 float32
// accumulator sets (lean form; the full form keeps 5 sets for 1 x 2 blocks and
// makes two passes over k).  One k-step = 256 sites = for every lane one uint4
// (four 32-site words) per plane and block, read from LDS with ds_read_b128
// and expanded four times (f = 0..3): 80 MFMAs per k-step and wavefront.  The
// planes come from the quad layout (king_common.h) by LDS-DMA, 16 KiB per
// k-step, kMfmaStages stages deep (king_common.h).  DESIGN.md 4.1 has the
// measurements behind the choices; archive/profiles/r01_mfma_microbench.txt the
// raw numbers.
//
// The kernel, king_mfma_kernel<FULL, SPLIT, N4, KIN>, is a short driver over phases, each
// a function of its own that is inlined into it (DESIGN.md 4.1 has the table):
//     take_work          which tile / piece / list entries the workgroup takes   (all)
//     next_segment       the next run of k-steps inside one tile                 (all)
//     hom_hom_pass       the fifth sum, from the het plane alone                 (FULL)
//     five_product_loop  the k loop on the quad layout                           (!N4)
//     four_product_loop  the k loop on the nibble layout                         (N4)
//     reduce_parts       park and sum the parts of a cut-up tile                 (SPLIT)
//     emit_full_records  two-sweep reservation and store         (FULL, no dense_counts;
//                        KIN = PI_HAT: decision and record of king_pihat.h, out of line)
//     store_counts       the six counts of every pair            (FULL, dense_counts)
//     store_kin          float32 kinship of every pair                    (KIN = matrix)
//     summarise_kin      histogram and nearest-relative keys of a tile    (KIN = summary)
//     count_relatives    lean_decide's test, then band and two atomics (KIN = relative counts)
//     lean_decide        threshold on the float sums, exact epilogue out of line (the rest)
// A k loop's statements are macros over its function's locals, defined and undefined
// inside that function.
#include <hip/hip_runtime.h>

#include "king_common.h"
#include "king_device.h"
#include "king_kin_summary.h"
#include "king_pihat.h"

// The LDS-DMA statements below write M0 and say so in their clobber lists; the
// compiler notes that it keeps no value of its own there (M0 is reserved).
#pragma clang diagnostic ignored "-Winline-asm"

namespace cuking {

namespace {

typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));

constexpr int kTile = 128;
constexpr int kStageU4 = 2 * 2 * 2 * kTile;  // sides x k-groups x planes x samples
constexpr int kPiecesPerWave = 4;            // 16 x 1 KiB per stage, 4 wavefronts
// Lean form (no LDS needed for a parked sum): more stages, at least the two it
// takes to hand stages over with one barrier per TWO k-steps.
// 10 x 16 KiB is the CU's whole LDS and puts 5.5 instead of 3.5 k-steps (8 stages)
// between a request and the hand-over that needs it: configs[2] 593 -> 590 ms,
// 40k x 100k 95.2 -> 94.7 ms, configs[1] (bitset in the Infinity Cache) equal
// (archive/experiments/exp25.sh).
constexpr int kStagesPaired = 10;
// The summary form's epilogue (summarise_kin()) reuses the stages: 256 keys of 8 bytes and the
// largest histogram's counts.  Both lean forms have 160 KiB.
constexpr uint32_t kMfmaSummaryLdsBytes = 2 * kTile * 8 + (CUKING_KIN_BINS_MAX + 3) * 4;
static_assert(kMfmaSummaryLdsBytes <= kStagesPaired * kStageU4 * 16 &&
                  kMfmaSummaryLdsBytes <= kMfmaN4LdsBytes,
              "the summary's LDS fits the stages of either lean form");

// v_bitop3_b32 truth tables over (het, hom_var, mask), index = 4 het + 2 hom + mask.
constexpr int kA = 0x08;  // hom-alt:  ~het &  hom & mask
constexpr int kR = 0x02;  // hom-ref:  ~het & ~hom & mask
constexpr int kH = 0x20;  // het:       het & ~hom & mask
constexpr int kD = 0x2A;  // defined:  ~(het & hom) & mask
constexpr int kY = 0x0A;  // A | R:    ~het & mask

// One operand fragment: plane KIND of four 32-site words at nibble position
// given by `mask` (an SGPR: a 32-bit literal would cost half a cycle more per
// instruction, tools/micro/mfma_fill).
template <int KIND>
__device__ __forceinline__ v8i frag(const uint4 het, const uint4 hom, uint32_t mask) {
  v8i r = {0, 0, 0, 0, 0, 0, 0, 0};
  r[0] = (int)__builtin_amdgcn_bitop3_b32(het.x, hom.x, mask, KIND);
  r[1] = (int)__builtin_amdgcn_bitop3_b32(het.y, hom.y, mask, KIND);
  r[2] = (int)__builtin_amdgcn_bitop3_b32(het.z, hom.z, mask, KIND);
  r[3] = (int)__builtin_amdgcn_bitop3_b32(het.w, hom.w, mask, KIND);
  return r;
}

// Nibble layout: a fragment is the stored dwords masked to one kind's bits.
__device__ __forceinline__ v8i nfrag(const uint4 w, uint32_t mask) {
  v8i r = {0, 0, 0, 0, 0, 0, 0, 0};
  r[0] = (int)(w.x & mask);
  r[1] = (int)(w.y & mask);
  r[2] = (int)(w.z & mask);
  r[3] = (int)(w.w & mask);
  return r;
}

__device__ __forceinline__ uint4 shr3(const uint4 w) {
  return make_uint4(w.x >> 3, w.y >> 3, w.z >> 3, w.w >> 3);
}

// acc += sum over the 64 sites of the fragment of a_site * b_site.  The E8M0
// scale 2^(1-F) on each side (F == 3 sits at position 0 again) undoes the
// 2^(F-1) of the expansion.  F == 1 needs none: scale operands 0 select the
// unscaled instruction, which holds the issue port 5 cycles less.
template <int F>
__device__ __forceinline__ v16f mma(const v8i a, const v8i b, const v16f c) {
  constexpr int scale = F == 0 ? 128 : F == 1 ? 0 : F == 2 ? 126 : 128;
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
      a, b, c, 4 /* A is fp4 */, 4 /* B is fp4 */, 0, scale, 0, scale);
}

// The exact lean epilogue of one register's pairs, out of line: it is reached
// for the few pairs that may pass the threshold, and inlined 64 times (with
// its recount loop and record append) it made the epilogue ~90 KB of code,
// more than the instruction cache.
__device__ __attribute__((noinline)) void lean_epilogue_call(
    const EmitCtx c, bool valid, uint32_t li, uint32_t lj, uint32_t het_i,
    uint32_t het_j, uint32_t both_het, uint32_t opp, uint32_t lane) {
  lean_epilogue_pair(c, valid, li, lj, het_i, het_j, both_het, opp, lane);
}

__device__ __attribute__((noinline)) void lean_epilogue_call_n4(
    const EmitCtxP c, bool valid, uint32_t li, uint32_t lj, uint32_t het_i,
    uint32_t het_j, uint32_t dd, int32_t q, uint32_t lane) {
  lean_epilogue_pair_n4(c, valid, li, lj, het_i, het_j, dd, q, lane);
}

// The exact epilogue of the relative-counts form (count_relatives()), out of line for the same
// reason: the pair's kinship from its four sums (kin_of_sums(), below), its band, and one
// atomic per end of the pair at the STORED samples' rows.  Per lane: no recount, so nothing
// needs the whole wavefront.
struct RelCtx {
  uint32_t *counts;
  uint32_t num;
  float thr[CUKING_REL_THRESHOLDS_MAX];
  const uint32_t *perm;  // the layout's sample order, or nullptr (TiledArgs::perm)
  uint32_t diag, num_rows, col_base;
};
template <bool N4>
__device__ __forceinline__ float kin_of_sums(float s0, float s1, float s2, float s3);
template <bool N4>
__device__ __attribute__((noinline)) void rel_count_call(const RelCtx c, bool maybe, uint32_t li,
                                                         uint32_t lj, float s0, float s1,
                                                         float s2, float s3) {
  if (!maybe) return;
  const uint32_t band = rel_band(c.thr, c.num, kin_of_sums<N4>(s0, s1, s2, s3));
  if (band == kRelNoBand) return;
  const uint32_t si = c.perm != nullptr ? c.perm[li] : li;
  const uint32_t sj = c.perm != nullptr ? c.perm[c.col_base + lj] : (c.diag ? lj : c.num_rows + lj);
  atomicAdd(c.counts + (size_t)si * c.num + band, 1u);
  atomicAdd(c.counts + (size_t)sj * c.num + band, 1u);
}

// Full form: a wavefront reserves the slots for ALL records of its 64 x 64 pairs
// with one atomic (one lane), out of line.  History: the per-pair append
// (atomicAdd in every lane, which the compiler turns into a wave-level
// aggregation with whole-wave-mode temporaries) inlined 64 times among ~500 live
// registers made the remainder-split instantiation return wrong sums for whole
// tiles whenever only a few lanes emitted (tools/fuzz_split.py seed 1 case 3);
// out of line per pair it was right but cost one atomic round trip per call --
// 11 ms per 10^6 records at configs[1] when most pairs pass.
// ... and the record itself (cuking.cu:297-313), out of line as well: the kernel
// around it has no registers to spare for 64 inlined copies.
template <class Ctx>
__device__ __attribute__((noinline)) void full_store_call(
    const Ctx c, uint32_t slot, uint32_t li, uint32_t lj, uint32_t het_i, uint32_t het_j,
    uint32_t both_het, uint32_t opp, uint32_t hom_hom) {
  if (slot >= c.max_results) {
    atomicMax(c.result_overflow, 1u);
    return;
  }
  const uint32_t ibs2 = hom_hom - opp + both_het;
  const uint32_t shared = het_i + het_j - both_het + hom_hom;
  cuking_result rec;
  record_pair(c, stored_row(c, li), stored_col(c, lj), &rec.sample_i, &rec.sample_j);
  rec.kin = king_kinship(het_i, het_j, both_het, opp);
  rec.ibs0 = opp;
  rec.ibs1 = shared - opp - ibs2;
  rec.ibs2 = ibs2;
  c.results[slot] = rec;
}

// PI_HAT form: the decision and the record, both out of line -- the fp64 pair math of
// king_pihat.h (divides included) is a few hundred instructions, and the kernel around the
// calls has no registers to spare.  ibs0/1/2 from the five sums as full_store_call has them.
struct PihatPair {
  uint32_t ibs0, ibs1, ibs2;
};
__device__ __forceinline__ PihatPair pihat_pair(uint32_t het_i, uint32_t het_j, uint32_t both_het,
                                                uint32_t opp, uint32_t hom_hom) {
  const uint32_t ibs2 = hom_hom - opp + both_het;
  const uint32_t shared = het_i + het_j - both_het + hom_hom;
  return PihatPair{opp, shared - opp - ibs2, ibs2};
}
__device__ __attribute__((noinline)) bool pihat_decide_call(const PihatArgs p, uint32_t het_i,
                                                            uint32_t het_j, uint32_t both_het,
                                                            uint32_t opp, uint32_t hom_hom) {
  const PihatPair c = pihat_pair(het_i, het_j, both_het, opp, hom_hom);
  return pihat_of_counts(p.e00, p.e01, p.e02, p.e11, p.e12, c.ibs0, c.ibs1, c.ibs2, p.flags) >
         p.min_pi_hat;
}
template <class Ctx>
__device__ __attribute__((noinline)) void pihat_store_call(
    const Ctx c, const PihatArgs p, uint32_t slot, uint32_t li, uint32_t lj, uint32_t het_i,
    uint32_t het_j, uint32_t both_het, uint32_t opp, uint32_t hom_hom) {
  if (slot >= c.max_results) {
    atomicMax(c.result_overflow, 1u);
    return;
  }
  const PihatPair n = pihat_pair(het_i, het_j, both_het, opp, hom_hom);
  cuking_result rec;
  record_pair(c, stored_row(c, li), stored_col(c, lj), &rec.sample_i, &rec.sample_j);
  rec.kin = pihat_of_counts(p.e00, p.e01, p.e02, p.e11, p.e12, n.ibs0, n.ibs1, n.ibs2, p.flags);
  rec.ibs0 = n.ibs0;
  rec.ibs1 = n.ibs1;
  rec.ibs2 = n.ibs2;
  c.results[slot] = rec;
}

__device__ __attribute__((noinline)) uint32_t reserve_slots(uint32_t *result_index, uint32_t n) {
  uint32_t base = 0;
  if ((threadIdx.x & 63) == 0)
    base = relaxed_add(result_index, n);
  return (uint32_t)__builtin_amdgcn_readfirstlane(base);
}

// `n` MFMAs, each followed by `v` VALU instructions (scheduling request).
#define CUKING_PACE(n, v)                                                      \
  _Pragma("unroll") for (int i_ = 0; i_ < (n); ++i_) {                         \
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                         \
    if ((v) > 0) __builtin_amdgcn_sched_group_barrier(0x002, (v), 0);          \
  }

// One LDS-DMA request: lane l's 16 bytes at SRC land at DST + 16 l (`lane16` of the
// function around it).  OFFSET ("" or " offset:1024") is the instruction's immediate, which
// moves source and destination alike.  Inline asm keeps it out of the compiler's wait-count
// bookkeeping (king_kernels.hip).
#define CUKING_LDS_DMA(DST, SRC, OFFSET)                                       \
  asm volatile("s_mov_b32 m0, %0\n\t"                                          \
               "s_nop 0\n\t"                                                   \
               "global_load_lds_dwordx4 %1, %2" OFFSET                         \
               :                                                               \
               : "s"(DST), "v"(lane16), "s"(SRC)                               \
               : "memory", "m0")

// Registers 4 r4 .. 4 r4 + 3 of an accumulator block as one 16-byte value, and back.
__device__ __forceinline__ float4 quarter(const v16f &v, int r4) {
  return make_float4(v[4 * r4], v[4 * r4 + 1], v[4 * r4 + 2], v[4 * r4 + 3]);
}
__device__ __forceinline__ void add_quarter(v16f &v, int r4, const float4 x) {
  v[4 * r4] += x.x;
  v[4 * r4 + 1] += x.y;
  v[4 * r4 + 2] += x.z;
  v[4 * r4 + 3] += x.w;
}
__device__ __forceinline__ void unpack(const float4 x, float *f) {
  f[0] = x.x;
  f[1] = x.y;
  f[2] = x.z;
  f[3] = x.w;
}
// A lane's 16-byte slots, lane-linear: of a parked fifth sum [block pair][4 registers][lane],
// and of a partial tile's slab [block pair][sum][4 registers][lane] (float4 units).
constexpr int park_slot(int bi, int bj, int r4) { return ((bi * 2 + bj) * 4 + r4) * 64; }
constexpr int slab_slot(int nsum, int bi, int bj, int q, int r4) {
  return (((bi * 2 + bj) * nsum + q) * 4 + r4) * 64;
}

// Tickets: one per workgroup and pass (the full form makes two).
__host__ __device__ inline size_t split_counter_bytes(uint32_t wgs) {
  return ((size_t)wgs * 2 * sizeof(uint32_t) + 255) / 256 * 256 + 256;
}
// ... and, in the last 256 bytes, the tile counter of a launch's dynamic tail.
__host__ __device__ inline size_t dyn_counter_index(uint32_t wgs) {
  return (split_counter_bytes(wgs) - 256) / sizeof(uint32_t);
}

// First work unit of split workgroup w: floor(w * units / wgs).
__device__ __forceinline__ uint64_t split_bound(uint64_t w, uint64_t units,
                                                uint32_t wgs) {
  return w * units / wgs;
}
// The split workgroup that owns unit u (needs units >= wgs).
__device__ __forceinline__ uint32_t split_owner(uint64_t u, uint64_t units,
                                                uint32_t wgs) {
  const uint32_t w = (uint32_t)(u * wgs / units);
  return split_bound(w + 1, units, wgs) <= u ? w + 1 : w;
}

// ---- The forms.  Five-product form: the lean form has 10 LDS stages and ONE stage barrier
// per two k-steps (five_product_loop()); the full form parks its fifth sum in the LDS behind
// the stages and keeps 6 stages with a barrier per k-step.  Four-product form: 5 stages of
// 32 KiB, every sum in registers.
constexpr int stages_of(bool full, bool n4) {
  return n4 ? kMfmaN4Stages : !full ? kStagesPaired : kMfmaStages;
}
constexpr int sums_of(bool full) { return full ? 5 : 4; }  // sums per pair
// ... of which the main loop keeps kNQ = 4 in its accumulators (five products:
// opp, bh, hi, hj; four products: hi / 2, hj / 2, dd, 4 q).  The full form's
// fifth sum, hom_hom, comes from a pass of its own in front of the main loop and
// waits for the epilogue PARKED in LDS (five products) or in 64 registers that
// the main loop does not touch (four products: `hh5`).
constexpr int kNQ = 4;

// ---- The phases of a workgroup, in the order king_mfma_kernel() (behind them) calls them:
// all inlined into the one kernel; each sees of the others what its parameters and its
// result say.
// What a workgroup has taken.  Wave-uniform.
struct Work {
  uint32_t bid;                // the tile within the launch (list / gate mode: the entry)
  uint32_t piece;              // SPLIT: the piece of the remainder
  bool listed;                 // list / gate mode: entries bid, bid + grid, ... < list_count
  uint32_t list_count;
  uint64_t unit_lo, unit_hi;   // the work units still to do; unit = (tile, k-step)
};
// The next run of k-steps inside one tile.  Wave-uniform.
struct Segment {
  uint32_t tile;               // within the launch
  uint32_t k_first, num_steps;
  uint32_t tr, tc;             // its row and column in the tile space
};
// Nibble masks, pinned to SGPRs.
struct NibbleMasks {
  uint32_t m1, m2, m4;
};
__device__ __forceinline__ NibbleMasks nibble_masks() {
  NibbleMasks m;
  asm volatile("s_mov_b32 %0, 0x11111111" : "=s"(m.m1));
  asm volatile("s_mov_b32 %0, 0x22222222" : "=s"(m.m2));
  asm volatile("s_mov_b32 %0, 0x44444444" : "=s"(m.m4));
  return m;
}
__device__ __forceinline__ uint32_t tile_steps_of(const TiledArgs &a) { return a.geo.k_words / 8; }

// Five-product full form: this lane's slots (park_slot()) of the parked fifth sum, behind
// the stages.
__device__ __forceinline__ float4 *park_slots(uint4 *const lds, const Lanes &l) {
  return reinterpret_cast<float4 *>(lds + stages_of(true, false) * kStageU4) +
         (size_t)l.wave * (4 * 4 * 64) + l.lane;
}

__device__ __forceinline__ void zero_acc(v16f (&acc)[2][2][kNQ]) {
#pragma unroll
  for (int bi = 0; bi < 2; ++bi)
#pragma unroll
    for (int bj = 0; bj < 2; ++bj)
#pragma unroll
      for (int q = 0; q < kNQ; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[bi][bj][q][r] = 0.f;
}

// Which tile (SPLIT: which piece) this workgroup takes.  False (uniform, before any barrier
// that others wait at) when there is none: the dynamic tail is through, the workgroup is
// padding, or the list is shorter than the grid.
template <bool SPLIT>
__device__ __forceinline__ bool take_work(const TiledArgs &a, uint4 *const lds, Work *w) {
  uint32_t bid = blockIdx.x;
  uint32_t piece = 0;
  if (a.dyn_tiles != 0 && blockIdx.x >= a.launch_tiles) {
    // dynamic tail (king_common.h): the next tile (SPLIT: the next piece of the
    // remainder) nobody has taken yet
    // (every workgroup of the tail asks exactly once: the last one to ask leaves
    // the counter ready for the next launch)
    uint32_t *slot = reinterpret_cast<uint32_t *>(lds);
    if (threadIdx.x == 0) {
      uint32_t *counter = a.split_counters + dyn_counter_index(a.split_wgs);
      const uint32_t asked = relaxed_add(counter, 1u);
      if (asked == a.dyn_wgs - 1)
        relaxed_store(counter, 0u);
      *slot = asked;
    }
    __syncthreads();
    const uint32_t t = __builtin_amdgcn_readfirstlane(*slot);
    __syncthreads();  // the word is stage memory from here on
    if (t >= a.dyn_tiles) return false;  // uniform
    if (SPLIT) piece = t; else bid = a.launch_tiles + t;
  } else
  // (SPLIT launches: the whole-tile workgroups in front take the patch order
  // when their count is a multiple of 8 x 32; the pieces behind them do not)
  if (a.xcd_chunk != 0 && (!SPLIT || blockIdx.x < a.split_whole)) {
    // xcd_chunk == 1: patches of 32 consecutive tiles dealt round-robin to the
    // XCDs (xcd_patch_tile()); otherwise one contiguous chunk of xcd_chunk tiles
    // per XCD.
    bid = a.xcd_chunk == 1 ? xcd_patch_tile(blockIdx.x)
                           : (blockIdx.x & 7) * a.xcd_chunk + (blockIdx.x >> 3);
    if (bid >= a.launch_tiles) return false;  // padding (uniform)
  }
  // Tile-list mode (king_common.h): entries bid, bid + grid, ... of the list.  The
  // persistent mode (gate != nullptr) walks the launch's own enumeration the same way:
  // units bid, bid + grid, ... of gate_count, or nothing at all when the gate is shut.
  w->listed = !SPLIT && (a.tile_list != nullptr || a.gate != nullptr);
  w->list_count = 0;
  if (w->listed) {
    if (a.gate != nullptr) {
      w->list_count = *a.gate != 0 ? a.gate_count : 0u;  // (uniform: a scalar load)
    } else {
      w->list_count = *a.tile_list_count;
      if (w->list_count > a.tile_list_cap) w->list_count = a.tile_list_cap;
    }
    // Workgroups are dealt round-robin to the 8 XCDs: give the ones that share an
    // XCD (and its L2) CONSECUTIVE entries of every round -- the list is in tile
    // order more or less, neighbours share row / column strips.
    if ((gridDim.x & 7) == 0) bid = (bid & 7) * (gridDim.x >> 3) + (bid >> 3);
    if (bid >= w->list_count) return false;  // uniform
  }
  w->bid = __builtin_amdgcn_readfirstlane(bid);
  w->piece = __builtin_amdgcn_readfirstlane(piece);

  // Work units [unit_lo, unit_hi) of this workgroup; unit = (tile, k-step).
  // SPLIT launches: the first split_whole workgroups take one whole tile each,
  // the remaining split_wgs ones cut the units of the last split_tiles tiles
  // into equal pieces (piece index `piece`).
  const uint32_t tile_steps = tile_steps_of(a);
  const uint64_t units = (uint64_t)a.split_tiles * tile_steps;      // of the cut-up tiles
  const uint64_t whole_units = SPLIT ? (uint64_t)a.split_whole * tile_steps : 0;
  const bool whole_wg = !SPLIT || blockIdx.x < a.split_whole;
  w->unit_lo = whole_wg ? (uint64_t)w->bid * tile_steps
                        : whole_units + split_bound(w->piece, units, a.split_wgs);
  w->unit_hi = whole_wg ? w->unit_lo + tile_steps
                        : whole_units + split_bound(w->piece + 1, units, a.split_wgs);
  return true;
}

// The walk over the workgroup's pieces: the next segment of its units, or false when it is
// through.  (List / gate mode: the next entry, behind a barrier.)
template <bool SPLIT>
__device__ __forceinline__ bool next_segment(const TiledArgs &a, Work *w, Segment *s) {
  const uint32_t tile_steps = tile_steps_of(a);
  while (true) {
    if (w->listed && w->unit_lo >= w->unit_hi) {
      w->bid += gridDim.x;
      if (w->bid >= w->list_count) return false;
      __syncthreads();  // every wavefront is through with the stages of the last tile
      w->unit_lo = (uint64_t)w->bid * tile_steps;
      w->unit_hi = w->unit_lo + tile_steps;
    }
    if (w->unit_lo >= w->unit_hi) return false;
    // Everything about the piece is wave-uniform; the 64-bit divisions behind it
    // are computed in vector registers, so pin the results to SGPRs (the SPLIT
    // instantiation otherwise runs out of VGPRs in the main loop and spills).
    const uint64_t unit_lo = w->unit_lo, unit_hi = w->unit_hi;
    s->tile =
        __builtin_amdgcn_readfirstlane((uint32_t)(unit_lo / tile_steps));  // within the launch
    s->k_first = __builtin_amdgcn_readfirstlane(
        (uint32_t)(unit_lo - (uint64_t)s->tile * tile_steps));
    s->num_steps = __builtin_amdgcn_readfirstlane(
        (unit_hi - unit_lo < (uint64_t)(tile_steps - s->k_first)) ? (uint32_t)(unit_hi - unit_lo)
                                                                 : tile_steps - s->k_first);
    w->unit_lo += s->num_steps;
    if (SPLIT) {
      // (the builtin returns int: the casts keep the low word from being sign-extended)
      w->unit_lo =
          ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(w->unit_lo >> 32)) << 32) |
          (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)w->unit_lo);
      w->unit_hi =
          ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(w->unit_hi >> 32)) << 32) |
          (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)w->unit_hi);
    }
    uint32_t tr, tc;
    if (!decode_tile(a, a.tile_begin + s->tile, &tr, &tc)) continue;  // uniform
    s->tr = __builtin_amdgcn_readfirstlane(tr);
    s->tc = __builtin_amdgcn_readfirstlane(tc);
    return true;
  }
}

// Full form: the fifth sum, hom_hom = (A|R)_i . (A|R)_j, in a pass of its own
// IN FRONT of the main loop.  Five sums for 2 x 2 blocks are 320 accumulator
// registers, more than the main loop can hold beside its fragments; but
// "homozygous and defined" is just ~het (missing and padding have the het bit
// set, cuking.cu:688-697), so this pass reads ONE plane, builds one fragment
// kind per side and issues 16 MFMAs per k-step against the main loop's 80.
// With so few MFMAs per byte the LDS-DMA requests and stage barriers of the
// main loop would dominate (measured: 1.9 ms of 8.8 at 10k x 100k), so every
// lane fetches its own operand words straight from the plane layout into
// registers, four k-steps ahead (512 B contiguous per half wavefront; each
// word is read by two wavefronts, from L2): no LDS, no barrier, the
// wavefronts drift freely.  The 64 result registers per lane are parked in
// the 64 KiB of LDS behind the stages until the epilogue (the workgroup owns
// the CU's whole 160 KiB anyway), so the main loop runs exactly as in the
// lean form.  (Round 1's full form made two passes of six products over
// 32-row blocks in the compiler's order: 10.3 ms at 10k x 100k against 7.0 ms
// lean.)
template <bool N4>
__device__ __forceinline__ void hom_hom_pass(const TiledArgs &a, const Segment &s, const Lanes &l,
                                             const NibbleMasks &m, uint4 *const lds,
                                             v16f (&hh)[2][2]) {
  const uint32_t g = l.g, lr = l.lr, wr = l.wy * 64, wc = l.wx * 64;
  const uint32_t s_stride = a.geo.s_stride, k_first = s.k_first, num_steps = s.num_steps;
  const uint32_t tr = s.tr, tc = s.tc;
  const uint32_t m1 = m.m1, m2 = m.m2, m4 = m.m4;
  constexpr int D = 4;  // k-steps in flight
#pragma unroll
  for (int bi = 0; bi < 2; ++bi)
#pragma unroll
    for (int bj = 0; bj < 2; ++bj)
#pragma unroll
      for (int r = 0; r < 16; ++r) hh[bi][bj][r] = 0.f;
  // The het plane, one uint4 per 128 sites and sample: plane 0 of the quad
  // layout (planes interleaved: quad stride 2 rows), or the het-only copy the
  // nibble layout carries behind its codes for this pass (quad stride 1).
  constexpr uint32_t HS = N4 ? 1 : 2;
  const uint4 *const h_base = N4 ? a.planes + (uint64_t)a.geo.k_words * s_stride : a.planes;
  const uint4 *lane_rows = h_base + (uint64_t)tr * kTile + (uint64_t)g * HS * s_stride + wr + lr;
  const uint4 *lane_cols = h_base + a.geo.col_base + (uint64_t)tc * kTile +
                           (uint64_t)g * HS * s_stride + wc + lr;
  uint4 Ha[D][2], Hb[D][2], Hs_a[2], Hs_b[2];
  v8i Pa[2], Pb[2], Qa[2], Qb[2];
  // het words of k-step min(step, last) (the repeats are masked out below)
#define CUKING_HH_LOAD(U, STEP)                                                \
  {                                                                            \
    uint32_t s_ = (STEP);                                                      \
    if (s_ >= num_steps) s_ = num_steps - 1;                                   \
    const uint64_t off_ = (uint64_t)(s_ + k_first) * 2 * HS * s_stride;        \
    _Pragma("unroll") for (int b = 0; b < 2; ++b) {                            \
      Ha[U][b] = lane_rows[off_ + b * 32];                                     \
      Hb[U][b] = lane_cols[off_ + b * 32];                                     \
    }                                                                          \
  }
#define CUKING_HH_FRAGS(X, SA, SB, MASK)                                       \
  _Pragma("unroll") for (int b = 0; b < 2; ++b) {                              \
    X##a[b] = frag<kY>(SA[b], SA[b], MASK);                                    \
    X##b[b] = frag<kY>(SB[b], SB[b], MASK);                                    \
  }
#define CUKING_HH_MMA(F, X)                                                    \
  _Pragma("unroll") for (int bi = 0; bi < 2; ++bi)                             \
  _Pragma("unroll") for (int bj = 0; bj < 2; ++bj)                             \
    hh[bi][bj] = mma<F>(X##a[bi], X##b[bj], hh[bi][bj]);
  // One k-step in four phases; while the four MFMAs of a phase issue, the
  // VALU builds the next phase's fragments into the other register set (the
  // last phase builds position 0 of the NEXT k-step, buffer UN).  A k-step
  // beyond the end gets zero masks: its fragments are empty.
#define CUKING_HH_KSTEP(U, UN)                                                 \
  {                                                                            \
    const bool live_ = step + (U) < num_steps;                                 \
    const bool next_ = step + (U) + 1 < num_steps;                             \
    const uint32_t k2_ = live_ ? m2 : 0u, k4_ = live_ ? m4 : 0u;               \
    const uint32_t k1_ = live_ ? m1 : 0u, n1_ = next_ ? m1 : 0u;               \
    CUKING_HH_FRAGS(Q, Ha[U], Hb[U], k2_)                                      \
    CUKING_HH_MMA(0, P)                                                        \
    CUKING_PACE(4, 4)                                                          \
    __builtin_amdgcn_sched_barrier(0);                                         \
    CUKING_HH_FRAGS(P, Ha[U], Hb[U], k4_)                                      \
    _Pragma("unroll") for (int b = 0; b < 2; ++b) {                            \
      Hs_a[b] = shr3(Ha[U][b]);                                                \
      Hs_b[b] = shr3(Hb[U][b]);                                                \
    }                                                                          \
    CUKING_HH_MMA(1, Q)                                                        \
    CUKING_PACE(4, 8)                                                          \
    __builtin_amdgcn_sched_barrier(0);                                         \
    CUKING_HH_FRAGS(Q, Hs_a, Hs_b, k1_)                                        \
    CUKING_HH_MMA(2, P)                                                        \
    CUKING_PACE(4, 4)                                                          \
    __builtin_amdgcn_sched_barrier(0);                                         \
    CUKING_HH_LOAD(U, step + D + (U))                                          \
    CUKING_HH_FRAGS(P, Ha[UN], Hb[UN], n1_)                                    \
    CUKING_HH_MMA(3, Q)                                                        \
    CUKING_PACE(4, 4)                                                          \
    __builtin_amdgcn_sched_barrier(0);                                         \
  }
  CUKING_HH_LOAD(0, 0)
  CUKING_HH_LOAD(1, 1)
  CUKING_HH_LOAD(2, 2)
  CUKING_HH_LOAD(3, 3)
  CUKING_HH_FRAGS(P, Ha[0], Hb[0], m1)
  for (uint32_t step = 0; step < num_steps; step += D) {
    CUKING_HH_KSTEP(0, 1)
    CUKING_HH_KSTEP(1, 2)
    CUKING_HH_KSTEP(2, 3)
    CUKING_HH_KSTEP(3, 0)
  }
#undef CUKING_HH_LOAD
#undef CUKING_HH_FRAGS
#undef CUKING_HH_MMA
#undef CUKING_HH_KSTEP
  if constexpr (!N4) {
    float4 *const park = park_slots(lds, l);
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
      for (int bj = 0; bj < 2; ++bj)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) park[park_slot(bi, bj, r4)] = quarter(hh[bi][bj], r4);
  }
  // (four-product form: the 64 registers stay where they are -- its main loop
  //  needs 256 accumulators + ~100, they fit beside)
  // (the prefetches beyond the end are in registers nobody reads; the
  //  compiler's own wait counts cover them before the main loop's hand-counted
  //  LDS-DMA starts: force that here)
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
}

// ---- Five products: the main loop over a segment's k-steps on the quad layout (file
// header), from the first LDS-DMA request to the last k-step's MFMAs.  FULL: six stages,
// hand-over every k-step; lean: ten, hand-over every two.  `lane16`, the lane's byte offset in
// a DMA row, is the driver's and carried from segment to segment through the pin below (worked
// out here per segment, the lean SPLIT form's k loop came out with three more LDS waits).
template <bool FULL>
__device__ __forceinline__ void five_product_loop(const TiledArgs &a, const Segment &s,
                                                  const Lanes &l, const NibbleMasks &m,
                                                  uint4 *const lds, uint32_t &lane16,
                                                  v16f (&acc)[2][2][kNQ]) {
  constexpr bool PAIRED = !FULL;
  constexpr int NSTAGE = stages_of(FULL, false);
  const uint32_t wave = l.wave, g = l.g, lr = l.lr, wr = l.wy * 64, wc = l.wx * 64;
  const uint32_t s_stride = a.geo.s_stride, k_first = s.k_first, num_steps = s.num_steps;
  const uint32_t m1 = m.m1, m2 = m.m2, m4 = m.m4;
  // This lane's operand rows inside a stage (uint4 units): rows / columns.
  uint32_t row_off = (0 * 2 + g) * 2 * kTile + wr + lr;
  uint32_t col_off = (1 * 2 + g) * 2 * kTile + wc + lr;
  const uint4 *g_rows = a.planes + (uint64_t)s.tr * kTile;
  const uint4 *g_cols = a.planes + a.geo.col_base + (uint64_t)s.tc * kTile;
  // LDS-DMA addressing.  Row `row` = 4 wave + r (1 KiB) of a stage is
  // (side, k-group, plane p, half seg) = (row >> 3, row >> 2 & 1, row >> 1 & 1,
  // row & 1): a wavefront's four requests share side and k-group, and r = 2 p +
  // seg, so that seg moves source and destination by the same 1 KiB -- the
  // instruction's immediate offset, which is added to both -- and only p needs
  // addresses of its own.  Per k-step that is one multiply for the wave-uniform
  // source row and a handful of scalar adds; `piece_addr` is called a phase ahead
  // of the requests, so that this arithmetic does not sit in the MFMA gaps that
  // already hold a request (it was 6-18 scalar instructions per request there).
  const uint32_t dma_side = wave >> 1, dma_kg = wave & 1;
  const uint4 *const g_wave = (dma_side ? g_cols : g_rows) +
                              ((uint64_t)(2 * k_first + dma_kg) * 2) * s_stride;
  const uint32_t l_wave = (uint32_t)(uintptr_t)(lds_void_ptr)(
      lds + ((dma_side * 2 + dma_kg) * 2) * kTile);
  struct PieceAddr { const uint4 *src[2]; uint32_t dst[2]; };
  // Source rows / LDS addresses of k-step min(step, last) -> buffer `buf`.
  // Clamping keeps the number of DMAs in flight the same in every iteration,
  // so one counted wait serves the whole loop; the repeats of the last step
  // land in a buffer nobody reads.
  auto piece_addr = [&](uint32_t step, uint32_t buf) {
    PieceAddr pa;
    if (step >= num_steps) step = num_steps - 1;
    pa.src[0] = g_wave + (uint64_t)step * 4 * s_stride;
    pa.src[1] = pa.src[0] + s_stride;
    pa.dst[0] = l_wave + buf * (kStageU4 * 16);
    pa.dst[1] = pa.dst[0] + kTile * 16;
    // materialised here, not where the requests are
    asm volatile("" : "+s"(pa.src[0]), "+s"(pa.src[1]), "+s"(pa.dst[0]), "+s"(pa.dst[1]));
    return pa;
  };
  // Request r of the four.
  auto issue_piece = [&](const PieceAddr &pa, int r) {
    if (r & 1) CUKING_LDS_DMA(pa.dst[r >> 1], pa.src[r >> 1], " offset:1024");
    else CUKING_LDS_DMA(pa.dst[r >> 1], pa.src[r >> 1], "");
  };
  auto issue_stage = [&](uint32_t step, uint32_t buf) {
    const PieceAddr pa = piece_addr(step, buf);
#pragma unroll
    for (int r = 0; r < kPiecesPerWave; ++r) issue_piece(pa, r);
  };
  // All but the NSTAGE - 2 youngest stages requested so far have landed, for
  // this wavefront (counted wait) and, after the barrier, for all of them;
  // every wavefront is also done reading the buffer the next request
  // overwrites.
  auto stage_sync = [&]() {
    // unpaired: the NSTAGE - 2 younger stages; paired: NSTAGE - 4 (see below)
    constexpr int younger = (PAIRED ? NSTAGE - 4 : NSTAGE - 2) * kPiecesPerWave;
    static_assert(younger < 64, "vmcnt is a 6-bit counter");
    __builtin_amdgcn_s_waitcnt(vmcnt_imm(younger));
    __syncthreads();
  };

  zero_acc(acc);  // (four products: behind the hom_hom pass, in front of the pins on hh5)
  // Raw words of the k-step: [block][plane] for the row and the column side.
  uint4 A[2][2], B[2][2];
#define CUKING_LOAD_RAW(BUF)                                                   \
  {                                                                            \
    const uint4 *l_rows_ = lds + (BUF) * kStageU4 + row_off;                   \
    const uint4 *l_cols_ = lds + (BUF) * kStageU4 + col_off;                   \
    _Pragma("unroll") for (int p = 0; p < 2; ++p) {                            \
      _Pragma("unroll") for (int b = 0; b < 2; ++b)                            \
        A[b][p] = l_rows_[p * kTile + b * 32];                                 \
      _Pragma("unroll") for (int b = 0; b < 2; ++b)                            \
        B[b][p] = l_cols_[p * kTile + b * 32];                                 \
    }                                                                          \
  }
// Fragment set X = planes A, R, H, D of (SA, SB) at the nibble position MASK.
#define CUKING_EXPAND(X, SA, SB, MASK)                                         \
  _Pragma("unroll") for (int b = 0; b < 2; ++b) {                              \
    X##a[b][0] = frag<kA>(SA[b][0], SA[b][1], MASK);                           \
    X##a[b][1] = frag<kR>(SA[b][0], SA[b][1], MASK);                           \
    X##a[b][2] = frag<kH>(SA[b][0], SA[b][1], MASK);                           \
    X##a[b][3] = frag<kD>(SA[b][0], SA[b][1], MASK);                           \
  }                                                                            \
  _Pragma("unroll") for (int b = 0; b < 2; ++b) {                              \
    X##b[b][0] = frag<kA>(SB[b][0], SB[b][1], MASK);                           \
    X##b[b][1] = frag<kR>(SB[b][0], SB[b][1], MASK);                           \
    X##b[b][2] = frag<kH>(SB[b][0], SB[b][1], MASK);                           \
    X##b[b][3] = frag<kD>(SB[b][0], SB[b][1], MASK);                           \
  }
// One plane product (fragment index PA of the rows x PB of the columns) for
// the four block pairs.
#define CUKING_MMA1(F, X, PA, PB, Q)                                           \
  _Pragma("unroll") for (int bi = 0; bi < 2; ++bi)                             \
  _Pragma("unroll") for (int bj = 0; bj < 2; ++bj)                             \
    acc[bi][bj][Q] = mma<F>(X##a[bi][PA], X##b[bj][PB], acc[bi][bj][Q]);
// opp (first half), bh, hi, hj: 16 MFMAs; then the second half of opp.
#define CUKING_MMA16(F, X)                                                     \
  CUKING_MMA1(F, X, 0, 1, 0) CUKING_MMA1(F, X, 2, 2, 1)                        \
  CUKING_MMA1(F, X, 2, 3, 2) CUKING_MMA1(F, X, 3, 2, 3)
#define CUKING_MMA4(F, X) CUKING_MMA1(F, X, 1, 0, 0)

  // Stage hand-over.  Unpaired (full form): stage s + NSTAGE - 1 is requested
  // while stage s is multiplied, into the buffer stage s - 1 left, and every
  // k-step ends with the counted wait + barrier.  Paired (lean form; written for 8 stages):
  // the barrier comes only at the end of ODD k-steps and then covers the next
  // TWO stages.  A request may only overwrite a buffer whose last readers are
  // separated from it by a barrier; the reads of stage k happen at the end of
  // k-step k - 1, so with barriers B(j) at the end of odd j an even k-step i
  // may request stage i + 7 (buffer of stage i - 1, read at the end of i - 2,
  // B(i - 1) in between) and an odd k-step i stage i + 5 (buffer of stage
  // i - 3, read at the end of i - 4, B(i - 2) in between).  Request order is
  // then 0..5, 7, 6, 9, 8, ...: when B(s) (s odd) waits for all but the 16
  // youngest requests of the wavefront, those are stages s+4, s+3, s+6, s+5,
  // i.e. stages s+1 and s+2 -- read at the end of k-steps s and s+1 -- have
  // landed: the same vmcnt(16) as the unpaired form.  (In general, N stages:
  // even k-steps request stage i + N - 1, odd ones i + N - 3, and the wait
  // leaves the N - 4 youngest stages in flight.)
  constexpr int kPrologueStages = PAIRED ? NSTAGE - 2 : NSTAGE - 1;
#pragma unroll
  for (int st = 0; st < kPrologueStages; ++st) issue_stage(st, st);
  stage_sync();

  // Software pipeline: while the MFMAs of fragment f issue, the VALU builds
  // fragment f + 1 into the other register set (an MFMA never reads a
  // register written just before it); behind the MFMAs of f = 3 come the
  // next k-step's stage hand-over, its LDS reads and its f = 0 fragment.
  // Pacing (tools/micro/mfma_fill): a scaled fp4 MFMA holds the issue port
  // 13 cycles (unscaled: 8) of its 32, a VALU instruction 4, so 4 (5) hide
  // behind one MFMA.  The k-step's four LDS-DMA requests go one each into
  // gaps without VALU work.
  v8i Xa[2][4], Xb[2][4], Ya[2][4], Yb[2][4];
  uint4 As[2][2], Bs[2][2];
  CUKING_LOAD_RAW(0)
  CUKING_EXPAND(X, A, B, m1)
  uint32_t buf = 0;  // buffer of the k-step being multiplied
  // The loop's per-lane invariants sit in registers from here on: a spill
  // reload whose first use is inside the loop would put the compiler's
  // s_waitcnt vmcnt(0) there, draining the DMA pipeline in every iteration.
  asm volatile("" : "+v"(row_off), "+v"(col_off), "+v"(lane16));
  // The raw words are dead after f = 1 (f = 2 and f = 3 read the shifted
  // copies): hand-over and LDS reads of the next k-step in phase f = 2, one
  // read behind each of its first eight MFMAs: configs[2] 594.5 ms; one per two
  // MFMAs 600.1, all in front of the phase 608.8 (archive/profiles/r02_mfma_stamps.txt).
#define CUKING_PHASE_F2(SYNC)                                                  \
    if (SYNC) stage_sync();                                                    \
    CUKING_LOAD_RAW(nbuf)                                                      \
    CUKING_EXPAND(Y, As, Bs, m1)                                               \
    CUKING_MMA16(2, X)                                                         \
    CUKING_MMA4(2, X)                                                          \
    _Pragma("unroll") for (int i_ = 0; i_ < 8; ++i_) {                         \
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                       \
      __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                       \
      __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);                       \
    }                                                                          \
    CUKING_PACE(8, 4) CUKING_PACE(4, 0)                                        \
    __builtin_amdgcn_sched_barrier(0);
#define CUKING_PHASE_F3(SYNC)                                                  \
    CUKING_EXPAND(X, A, B, m1)                                                 \
    CUKING_MMA16(3, Y)                                                         \
    CUKING_MMA4(3, Y)                                                          \
    CUKING_PACE(4, 0) CUKING_PACE(16, 4)                                       \
    __builtin_amdgcn_sched_barrier(0);
  // One k-step.  Its four requests go to the addresses the k-step before it
  // worked out (`pa`); in phase f = 3, where the MFMA gaps have room for scalar
  // instructions, it works out those of the NEXT k-step, which requests stage
  // STEP + 1 + NAHEAD into the buffer NBACK behind its own.  SYNC = hand stages
  // over (wait + barrier) before the next k-step's LDS reads.
#define CUKING_KSTEP(STEP, SYNC, NAHEAD, NBACK)                                \
  {                                                                            \
    const uint32_t nbuf = buf == NSTAGE - 1 ? 0 : buf + 1;                     \
    const PieceAddr pa_ = pa;                                                  \
    /* f = 0 multiplies, f = 1 is built */                                     \
    CUKING_EXPAND(Y, A, B, m2)                                                 \
    CUKING_MMA16(0, X)                                                         \
    CUKING_PACE(16, 4)                                                         \
    __builtin_amdgcn_sched_barrier(0);                                         \
    _Pragma("unroll") for (int r = 0; r < 4; ++r) {                            \
      issue_piece(pa_, r);                                                     \
      acc[r >> 1][r & 1][0] =                                                  \
          mma<0>(Xa[r >> 1][1], Xb[r & 1][0], acc[r >> 1][r & 1][0]);          \
      __builtin_amdgcn_sched_barrier(0);                                       \
    }                                                                          \
    /* f = 1 multiplies (unscaled), f = 2 and the shifted words are built */   \
    CUKING_EXPAND(X, A, B, m4)                                                 \
    _Pragma("unroll") for (int b = 0; b < 2; ++b)                              \
    _Pragma("unroll") for (int p = 0; p < 2; ++p) {                            \
      As[b][p] = shr3(A[b][p]);                                                \
      Bs[b][p] = shr3(B[b][p]);                                                \
    }                                                                          \
    CUKING_MMA16(1, Y)                                                         \
    CUKING_MMA4(1, Y)                                                          \
    CUKING_PACE(20, 5)                                                         \
    __builtin_amdgcn_sched_barrier(0);                                         \
    CUKING_PHASE_F2(SYNC)                                                      \
    pa = piece_addr((STEP) + 1 + (NAHEAD),                                     \
                    nbuf >= (NBACK) ? nbuf - (NBACK) : nbuf + NSTAGE - (NBACK)); \
    CUKING_PHASE_F3(SYNC)                                                      \
    buf = nbuf;                                                                \
  }
  // (the first k-step requests stage NSTAGE - 1 into the buffer behind its own)
  PieceAddr pa = piece_addr(NSTAGE - 1, buf >= 1 ? buf - 1 : buf + NSTAGE - 1);
  if constexpr (PAIRED) {
    // even k-steps request stage + NSTAGE - 1 one buffer back, odd ones
    // stage + NSTAGE - 3 three buffers back
    uint32_t step = 0;
    for (; step + 2 < num_steps; step += 2) {
      CUKING_KSTEP(step, false, NSTAGE - 3, 3)
      CUKING_KSTEP(step + 1, true, NSTAGE - 1, 1)
    }
    if (step + 1 < num_steps) CUKING_KSTEP(step, false, NSTAGE - 3, 3)
  } else {
    for (uint32_t step = 0; step + 1 < num_steps; ++step)
      CUKING_KSTEP(step, true, NSTAGE - 1, 1)
  }
#undef CUKING_KSTEP
#undef CUKING_PHASE_F2
#undef CUKING_PHASE_F3
  // last k-step: nothing left to fetch
  CUKING_EXPAND(Y, A, B, m2)
  CUKING_MMA16(0, X)
  CUKING_MMA4(0, X)
  CUKING_EXPAND(X, A, B, m4)
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      As[b][p] = shr3(A[b][p]);
      Bs[b][p] = shr3(B[b][p]);
    }
  CUKING_MMA16(1, Y)
  CUKING_MMA4(1, Y)
  CUKING_EXPAND(Y, As, Bs, m1)
  CUKING_MMA16(2, X)
  CUKING_MMA4(2, X)
  CUKING_MMA16(3, Y)
  CUKING_MMA4(3, Y)
#undef CUKING_LOAD_RAW
#undef CUKING_EXPAND
#undef CUKING_MMA1
#undef CUKING_MMA16
#undef CUKING_MMA4
}

// ---- Four products ------------------------------------------------------
// With D = defined, H = het, Y = hom-ref or hom-alt, T = (hom-ref) - (hom-alt):
//     hi = H_i.D_j    hj = D_i.H_j    dd = D_i.D_j    q = T_i.T_j
// and  2 bh - 4 opp - hi - hj = hi + hj - 2 dd + 2 q   (kinship's numerator),
//      bh - hom_hom = hi + hj - dd,   hom_hom - 2 opp = q,
// so four MFMAs per block pair and 64 sites instead of five give the
// threshold decision (the minimum: {numerator, hi, hj} is not in the span of
// three rank-1 products), and one more sum -- hom_hom, recounted for the few
// emitted pairs (lean) or from the pass in front of this loop (full form: the
// same het-plane pass as the five-product kernel's, reading a het-only copy
// behind the codes; a fifth product Y_i.Y_j inside this loop would need 320
// accumulator registers, which the compiler then shuffles between the two
// halves of the register file around every MFMA, and a pass of its own over
// the staged codes moves all the bytes again for a quarter of the MFMAs:
// 3.2 ms of 8.8 at 10k x 100k) -- gives bh and opp.
// T needs a sign: the nibble layout (king_common.h) stores one fp4 code per
// site, H at bit 0 (0.5), D at bit 1 (1.0), Y at bit 2 (2.0), hom-alt in the
// SIGN bit, so that every fragment is ONE v_and_b32 of a stored dword with a
// constant (T: 0xC -> +-2.0) -- no bit-position passes, no shifted copies, no
// block scales: all MFMAs are the unscaled instruction, and each product
// carries a constant power of two (hi, hj: 1/2; q, hom_hom: 4) that the
// epilogue takes out exactly.  Per k-step (256 sites, 4 slices of 64) and
// wavefront: 64 MFMAs, 192 v_and (3.0 per MFMA; five products: 80 / 288),
// 16 ds_read_b128, 8 LDS-DMA requests of 1 KiB (twice the bytes).
//
// Pipeline (per slice c = 16 or 20 MFMAs): fragments are NOT double
// buffered; a fragment kind is rebuilt for slice c + 1 in the MFMA group
// behind its last use in slice c (group order hi, hj, dd, q[, hom_hom]), the
// raw words of slice c + 1 sit in the second raw buffer, and the LDS reads of
// slice c + 2 go into the buffer slice c has finished with.
template <bool FULL>
__device__ __forceinline__ void four_product_loop(const TiledArgs &a, const Segment &s,
                                                  const Lanes &l, const NibbleMasks &m,
                                                  uint4 *const lds, v16f (&acc)[2][2][kNQ],
                                                  v16f (&hh5)[2][2]) {
  constexpr bool HH5 = FULL;
  constexpr int NSTAGE = stages_of(FULL, true);
  const uint32_t wave = l.wave, g = l.g, lr = l.lr, wr = l.wy * 64, wc = l.wx * 64;
  const uint32_t s_stride = a.geo.s_stride, k_first = s.k_first, num_steps = s.num_steps;
  const uint32_t m1 = m.m1, m2 = m.m2;
  uint32_t lane16 = l.lane * 16;           // byte offset of the lane in a DMA row
  const uint32_t dma_side = wave >> 1, dma_kg = wave & 1;
  const uint4 *g_rows = a.planes + (uint64_t)s.tr * kTile;
  const uint4 *g_cols = a.planes + a.geo.col_base + (uint64_t)s.tc * kTile;
  constexpr int kSliceU4 = kTile;                  // one slice of one (side, k-group)
  constexpr int kStageN4 = 2 * 2 * 4 * kSliceU4;   // uint4 per stage (32 KiB)
  uint32_t mT;
  asm volatile("s_mov_b32 %0, 0xcccccccc" : "=s"(mT));
  const uint32_t mH = m1, mD = m2;
  // DMA: wavefront (side, k-group) fetches that quarter of a stage: 4 slices x
  // 2 halves of 64 samples, 1 KiB each.  Slice c of k-step s is group
  // 8 s + 4 kg + c of the layout.
  const uint4 *const g_wave4 = (dma_side ? g_cols : g_rows) +
                               (uint64_t)(8 * k_first + 4 * dma_kg) * s_stride;
  const uint32_t l_wave4 = (uint32_t)(uintptr_t)(lds_void_ptr)(
      lds + ((dma_side * 2 + dma_kg) * 4) * kSliceU4);
  struct N4Addr { const uint4 *src; uint32_t dst; };
  auto n4_addr = [&](uint32_t step, uint32_t buf) {
    N4Addr pa;
    if (step >= num_steps) step = num_steps - 1;  // (clamped repeats: see piece_addr)
    pa.src = g_wave4 + (uint64_t)step * 8 * s_stride;
    pa.dst = l_wave4 + buf * (kStageN4 * 16);
    asm volatile("" : "+s"(pa.src), "+s"(pa.dst));
    return pa;
  };
  // ... of the stage after the one `pa` names: one k-step further unless that was
  // the last (then the same rows again: clamped repeats), into buffer `buf` --
  // a compare, a select and two adds instead of n4_addr's 64-bit multiply chain
  // (65 cycles of a k-step in the stamps, profiles/r03_stamps_n4.txt).
  const uint32_t kstep_bytes = 8 * s_stride * 16;  // (< 2^32: 128 B x stored samples)
  auto n4_next = [&](const N4Addr &cur, uint32_t step, uint32_t buf) {
    N4Addr pa;
    const uint32_t adv = step < num_steps ? kstep_bytes : 0u;
    pa.src = reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(cur.src) + adv);
    pa.dst = l_wave4 + buf * (kStageN4 * 16);
    asm volatile("" : "+s"(pa.src), "+s"(pa.dst));
    return pa;
  };
  auto n4_issue = [&](const N4Addr &pa, int c, int half) {
    const uint4 *src = pa.src + (uint64_t)c * s_stride;
    const uint32_t dst = pa.dst + c * (kSliceU4 * 16);
    if (half) CUKING_LDS_DMA(dst, src, " offset:1024");
    else CUKING_LDS_DMA(dst, src, "");
  };
  // Stage hand-over, once per k-step (in its third slice, before the first LDS
  // read of the next stage).  Requests of this wavefront still in flight then:
  // stages s + 1 .. s + 3 and the 4 requests of stage s + 4 that slices 0 and 1
  // have issued; stage s + 1 has landed when all but the 20 youngest have.
  auto n4_sync = [&]() {
    __builtin_amdgcn_s_waitcnt(vmcnt_imm(2 * 8 + 4));
    __syncthreads();
  };
  // Stages 0 .. NSTAGE - 2 requested, stage 0 landed.
  auto n4_prologue = [&]() {
#pragma unroll
    for (int st = 0; st < NSTAGE - 1; ++st) {
      const N4Addr pa0 = n4_addr(st, st);
#pragma unroll
      for (int r = 0; r < 8; ++r) n4_issue(pa0, r >> 1, r & 1);
    }
    __builtin_amdgcn_s_waitcnt(vmcnt_imm(3 * 8));
    __syncthreads();
  };

  // This lane's operand rows inside a stage (uint4 units): rows / columns.
  uint32_t row_off4 = (0 * 2 + g) * 4 * kSliceU4 + wr + lr;
  uint32_t col_off4 = (1 * 2 + g) * 4 * kSliceU4 + wc + lr;
  asm volatile("" : "+v"(row_off4), "+v"(col_off4), "+v"(lane16));
  uint4 RA[2][2], RB[2][2];  // raw words [raw buffer][block]
  // fragment kinds: 0 H, 1 D, 2 T, 3 Y
  v8i Fa[4][2], Fb[4][2];
#define N4_READ(RB_, BUF, C)                                                   \
  {                                                                            \
    const uint4 *l_rows_ = lds + (BUF) * kStageN4 + row_off4 + (C) * kSliceU4; \
    const uint4 *l_cols_ = lds + (BUF) * kStageN4 + col_off4 + (C) * kSliceU4; \
    _Pragma("unroll") for (int b = 0; b < 2; ++b) RA[RB_][b] = l_rows_[b * 32]; \
    _Pragma("unroll") for (int b = 0; b < 2; ++b) RB[RB_][b] = l_cols_[b * 32]; \
  }
// Fragment builds are plain ANDs: nothing orders them against the MFMA groups
// but data.  Left alone, the compiler gathers every build that reads a raw
// buffer into the group that first touches it (60 ANDs behind 4 MFMAs, none
// behind the next 12).  N4_PIN passes values through an empty asm statement:
// a build cannot move above the pin of its input nor below the pin of its
// result, which ties it to the group it is written in.
#define N4_PIN4(W) asm volatile("" : "+v"((W).x), "+v"((W).y), "+v"((W).z), "+v"((W).w));
#define N4_PINF(F) asm volatile("" : "+v"((F)[0]), "+v"((F)[1]), "+v"((F)[2]), "+v"((F)[3]));
#define N4_PIN_RAW_A(RB_) _Pragma("unroll") for (int b = 0; b < 2; ++b) N4_PIN4(RA[RB_][b])
#define N4_PIN_RAW_B(RB_) _Pragma("unroll") for (int b = 0; b < 2; ++b) N4_PIN4(RB[RB_][b])
#define N4_PIN_A(K) _Pragma("unroll") for (int b = 0; b < 2; ++b) N4_PINF(Fa[K][b])
#define N4_PIN_B(K) _Pragma("unroll") for (int b = 0; b < 2; ++b) N4_PINF(Fb[K][b])
#define N4_BUILD_A(K, RB_, MASK)                                               \
  _Pragma("unroll") for (int b = 0; b < 2; ++b) Fa[K][b] = nfrag(RA[RB_][b], MASK);
#define N4_BUILD_B(K, RB_, MASK)                                               \
  _Pragma("unroll") for (int b = 0; b < 2; ++b) Fb[K][b] = nfrag(RB[RB_][b], MASK);
// product Q = kind KA of the rows x kind KB of the columns, four block pairs
#define N4_MMA(Q, KA, KB)                                                      \
  _Pragma("unroll") for (int bi = 0; bi < 2; ++bi)                             \
  _Pragma("unroll") for (int bj = 0; bj < 2; ++bj)                             \
    acc[bi][bj][Q] = mma<1>(Fa[KA][bi], Fb[KB][bj], acc[bi][bj][Q]);
// A group of four MFMAs that also carries the slice's two DMA requests (in gaps
// of their own) and the H columns of the next slice.
#define N4_DMA_GROUP(Q, K, NXT, C)                                             \
  _Pragma("unroll") for (int r = 0; r < 2; ++r) {                              \
    n4_issue(pa, C, r);                                                        \
    acc[0][r][Q] = mma<1>(Fa[K][0], Fb[K][r], acc[0][r][Q]);                   \
    __builtin_amdgcn_sched_barrier(0);                                         \
  }                                                                            \
  N4_PIN_RAW_B(NXT)                                                            \
  N4_BUILD_B(0, NXT, mH)                                                       \
  _Pragma("unroll") for (int r = 0; r < 2; ++r)                                \
    acc[1][r][Q] = mma<1>(Fa[K][1], Fb[K][r], acc[1][r][Q]);                   \
  CUKING_PACE(2, 4)                                                            \
  N4_PIN_B(0)                                                                  \
  __builtin_amdgcn_sched_barrier(0);
// A group that issues the LDS reads of the slice after next (behind the stage
// hand-over if SYNC) and builds the H rows of the next slice.
#define N4_READ_GROUP(Q, KA, KB, CUR, NXT, RBUF, RSLICE, SYNC)                 \
  if (SYNC) n4_sync();                                                         \
  N4_READ(CUR, RBUF, RSLICE)                                                   \
  N4_PIN_RAW_A(NXT)                                                            \
  N4_BUILD_A(0, NXT, mH)                                                       \
  N4_MMA(Q, KA, KB)                                                            \
  _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) {                           \
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                         \
    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                         \
    __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);                         \
  }                                                                            \
  N4_PIN_A(0)                                                                  \
  __builtin_amdgcn_sched_barrier(0);
// The last group of a slice: D of the next slice, columns first (the next
// slice's first MFMAs read them).
#define N4_LAST_GROUP(Q, KA, KB, NXT)                                          \
  N4_PIN_RAW_A(NXT) N4_PIN_RAW_B(NXT)                                          \
  N4_BUILD_B(1, NXT, mD) N4_BUILD_A(1, NXT, mD)                                \
  N4_MMA(Q, KA, KB)                                                            \
  CUKING_PACE(4, 4)                                                            \
  N4_PIN_B(1) N4_PIN_A(1)                                                      \
  __builtin_amdgcn_sched_barrier(0);
// One slice.  CUR / NXT: raw buffers of this and the next slice; (RBUF, RSLICE):
// stage buffer and slice whose raw words are read into CUR once this slice is
// through with them (the slice after next); C: which slice's two DMA requests
// go out; SYNC: stage hand-over in front of the reads.
#define N4_SLICE(CUR, NXT, RBUF, RSLICE, SYNC, C)                              \
  {                                                                            \
    /* hi = H_i.D_j; T of this slice from its own raw words */                 \
    N4_PIN_RAW_A(CUR) N4_PIN_RAW_B(CUR)                                        \
    N4_BUILD_A(2, CUR, mT) N4_BUILD_B(2, CUR, mT)                              \
    N4_MMA(0, 0, 1)                                                            \
    /* (last slice: the next k-step's request addresses -- a dependent chain   \
       of ~10 scalar instructions -- among this group's MFMAs, not behind the  \
       k-step where nothing covers them) */                                    \
    if ((C) == 3) pa_next = n4_next(pa, step + NSTAGE, buf);                   \
    CUKING_PACE(4, 4)                                                          \
    N4_PIN_A(2) N4_PIN_B(2)                                                    \
    __builtin_amdgcn_sched_barrier(0);                                         \
    /* hj = D_i.H_j */                                                         \
    N4_READ_GROUP(1, 1, 0, CUR, NXT, RBUF, RSLICE, SYNC)                       \
    /* dd = D_i.D_j */                                                         \
    N4_DMA_GROUP(2, 1, NXT, C)                                                 \
    /* q = T_i.T_j */                                                          \
    N4_LAST_GROUP(3, 2, 2, NXT)                                                \
  }
  zero_acc(acc);
  if constexpr (HH5) {
    // 320 accumulator-like registers for a 256-entry accumulator file: say
    // which 64 live in the other half (left to itself the compiler moves some
    // of each through v_accvgpr copies around every MFMA of the split
    // instantiation's main loop: 368 copies per k-step).
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
      for (int bj = 0; bj < 2; ++bj) {
        asm volatile("" : "+v"(hh5[bi][bj]));
#pragma unroll
        for (int q = 0; q < kNQ; ++q) asm volatile("" : "+a"(acc[bi][bj][q]));
      }
  }
  n4_prologue();
  N4_READ(0, 0, 0)
  N4_READ(1, 0, 1)
  N4_BUILD_A(0, 0, mH) N4_BUILD_B(0, 0, mH)
  N4_BUILD_A(1, 0, mD) N4_BUILD_B(1, 0, mD)
  uint32_t buf = 0;  // buffer of the k-step being multiplied
  // k-step s requests stage s + NSTAGE - 1 into the buffer stage s - 1 left
  // (all its reads were issued before the hand-over of k-step s - 1)
  N4Addr pa = n4_addr(NSTAGE - 1, NSTAGE - 1);
  // One k-step; four per loop trip (the trip's back edge and counter updates cost
  // ~100 cycles with nothing to cover them: stamps, profiles/r03_stamps_n4.txt;
  // 1, 2, 4 k-steps per trip: configs[2] 540 -> 529 -> 526 ms).
#define N4_KSTEP                                                               \
  {                                                                            \
    const uint32_t nbuf = buf == NSTAGE - 1 ? 0 : buf + 1;                     \
    N4Addr pa_next;                                                            \
    N4_SLICE(0, 1, buf, 2, false, 0)                                           \
    N4_SLICE(1, 0, buf, 3, false, 1)                                           \
    N4_SLICE(0, 1, nbuf, 0, true, 2)                                           \
    N4_SLICE(1, 0, nbuf, 1, false, 3)                                          \
    pa = pa_next;                                                              \
    buf = nbuf;                                                                \
    ++step;                                                                    \
  }
  uint32_t step = 0;
  while (step + 3 < num_steps) {
    N4_KSTEP
    N4_KSTEP
    N4_KSTEP
    N4_KSTEP
  }
  while (step < num_steps) N4_KSTEP
#undef N4_KSTEP
#undef N4_READ
#undef N4_PIN4
#undef N4_PINF
#undef N4_PIN_RAW_A
#undef N4_PIN_RAW_B
#undef N4_PIN_A
#undef N4_PIN_B
#undef N4_BUILD_A
#undef N4_BUILD_B
#undef N4_MMA
#undef N4_DMA_GROUP
#undef N4_READ_GROUP
#undef N4_LAST_GROUP
#undef N4_SLICE
}

// SPLIT, a partial tile: park this part in its own slab (16-byte stores,
// lane-linear [wave][block pair][sum][4 registers][lane]), then take a
// ticket of the tile.  Slab of a part: 2 * workgroup + (0 for the piece in
// the workgroup's first tile, 1 for the piece in its second).  The workgroup that
// delivers the tile's last part adds the others to its own and runs the epilogue (true);
// the others are through with the tile.  `park`: the five-product full form's fifth sum.
template <bool FULL, bool N4>
__device__ __forceinline__ bool reduce_parts(const TiledArgs &a, const uint32_t piece,
                                             const Segment &s, const Lanes &l, uint4 *const lds,
                                             float4 *const park, v16f (&acc)[2][2][kNQ],
                                             v16f (&hh5)[2][2]) {
  constexpr int NSUM = sums_of(FULL);
  constexpr bool HH5 = FULL && N4;
  constexpr size_t kSlabU4 = 4 * 4 * 4 * 4 * 64;          // uint4 per slab (lean)
  constexpr size_t kPassU4 = 4 * 2 * 2 * NSUM * 4 * 64;   // ... of this form
  static_assert(kPassU4 <= kSlabU4 * 5 / 4, "slab size");
  const uint32_t tile_steps = tile_steps_of(a);
  const uint64_t units = (uint64_t)a.split_tiles * tile_steps;  // of the cut-up tiles
  // (positions inside the cut-up part of the launch: tile and units count
  // from its first tile)
  const uint32_t cut_tile = s.tile - a.split_whole;
  const uint64_t first_unit = (uint64_t)cut_tile * tile_steps;
  const uint64_t my_first = split_bound(piece, units, a.split_wgs);
  const uint32_t my_slab = 2 * piece + (my_first / tile_steps == cut_tile ? 0 : 1);
  float4 *slabs = reinterpret_cast<float4 *>(a.split_scratch);
  constexpr size_t kSlabStride = kSlabU4 * 5 / 4;  // sized for the full form
  {
    // Write-through (sc1) 16-byte stores: the data is in memory when the
    // wait below returns, so no release fence (which would write back the
    // whole L2: tens of microseconds with 256 KiB freshly dirtied).
    typedef uint32_t v4u __attribute__((ext_vector_type(4)));
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        slabs + my_slab * kSlabStride, 0, (int)(kPassU4 * 16), 0x00020000);
    const int base = (int)((l.wave * (2 * 2 * NSUM * 4 * 64) + l.lane) * 16);
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
      for (int bj = 0; bj < 2; ++bj)
#pragma unroll
        for (int q = 0; q < NSUM; ++q)
#pragma unroll
          for (int r4 = 0; r4 < 4; ++r4) {
            float4 f;
            if (q < kNQ) f = quarter(acc[bi][bj][q], r4);
            else if constexpr (HH5) f = quarter(hh5[bi][bj], r4);
            else f = park[park_slot(bi, bj, r4)];
            const v4u v = {__float_as_uint(f.x), __float_as_uint(f.y), __float_as_uint(f.z),
                           __float_as_uint(f.w)};
            __builtin_amdgcn_raw_buffer_store_b128(
                v, rsrc, base + slab_slot(NSUM, bi, bj, q, r4) * 16, 0, 16 /* sc1 */);
          }
  }
  // Every wavefront's stores are done (and written through), then the
  // ticket (cdna_hip_programming.md, Guideline 16: sc1 payload + counter).
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  uint32_t *flag = reinterpret_cast<uint32_t *>(lds);  // stages are idle now
  const uint32_t w_first = split_owner(first_unit, units, a.split_wgs);
  const uint32_t w_last = split_owner(first_unit + tile_steps - 1, units, a.split_wgs);
  if (threadIdx.x == 0) {
    // One counter per workgroup (and pass): a workgroup owns the first unit
    // of at most one tile that continues into the next workgroup.
    uint32_t *counter = a.split_counters + w_first;
    const uint32_t ticket = relaxed_add(counter, 1u);
    const bool last = ticket == w_last - w_first;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      *counter = 0;  // ready for the next launch
    }
    *flag = last ? 1u : 0u;
  }
  __syncthreads();
  const bool last = *flag != 0;
  __syncthreads();  // the flag word is stage memory again after this
  if (!last) return false;
  // Totals: this part is still in registers, the others come from their slabs.
  for (uint32_t w = w_first; w <= w_last; ++w) {
    if (w == piece) continue;
    const uint32_t slab =
        2 * w + (split_bound(w, units, a.split_wgs) / tile_steps == cut_tile ? 0 : 1);
    const float4 *src =
        slabs + slab * kSlabStride + (size_t)l.wave * (2 * 2 * NSUM * 4 * 64) + l.lane;
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
      for (int bj = 0; bj < 2; ++bj)
#pragma unroll
        for (int q = 0; q < NSUM; ++q)
#pragma unroll
          for (int r4 = 0; r4 < 4; ++r4) {
            const float4 v = src[slab_slot(NSUM, bi, bj, q, r4)];
            if (q < kNQ) {
              add_quarter(acc[bi][bj][q], r4, v);
            } else if constexpr (HH5) {
              add_quarter(hh5[bi][bj], r4, v);
            } else {
              float4 &h = park[park_slot(bi, bj, r4)];
              h = make_float4(h.x + v.x, h.y + v.y, h.z + v.z, h.w + v.w);
            }
          }
  }
  return true;
}

// ---- Epilogues: kinship, threshold, append (cuking.cu:284-313).  C layout of the 32 x 32
// MFMA: column = lane & 31, row = c_row(r, lane >> 5).
// Row (column) within the block of register r of block row bi (of block column bj), from the
// wavefront's first row (column) `row0` (`col0`).  The full form's epilogues work the origin out
// per pair, the lean ones ONCE in front of their loops (pair_origin()); the other way round,
// the k loops of the full four-product forms and of the unsplit dense-kinship forms each came
// out of the compiler with one to four more LDS waits.
struct PairOrigin {
  uint32_t row0, col0;
};
__device__ __forceinline__ PairOrigin pair_origin(const Segment &s, const Lanes &l) {
  return PairOrigin{s.tr * kTile + l.wy * 64, s.tc * kTile + l.wx * 64};
}
__device__ __forceinline__ uint32_t pair_row(const PairOrigin &o, const Lanes &l, int bi, int r) {
  return o.row0 + bi * 32 + c_row(r, l.g);
}
__device__ __forceinline__ uint32_t pair_col(const PairOrigin &o, const Lanes &l, int bj) {
  return o.col0 + bj * 32 + l.lr;
}
// cuking.cu:199 plus the tile padding (`diag` = 1: the pairs (i, i) as well)
__device__ __forceinline__ bool pair_valid(const TiledArgs &a, uint32_t li, uint32_t lj,
                                           uint32_t diag = 0) {
  return li < a.geo.num_rows && lj < a.geo.num_cols && a.i_begin + li < a.j_begin + lj + diag;
}
template <bool N4>
__device__ __forceinline__ auto emit_ctx_of(const TiledArgs &a) {
  if constexpr (N4) return make_emit_ctx_p(a);
  else return make_emit_ctx(a);
}

// The five sums of pair (bi, bj, r) as integers (full form).  Five products: they are the
// accumulators (hom_hom parked, `parked`).  Four products: hi / 2, hj / 2, dd,
// 4 q (and hom_hom in hh5) are, and bh = hi + hj - dd + hom_hom,
// opp = (hom_hom - q) / 2.  (Full form only: the lean forms never run hom_hom_pass, their
// `hh5` is a name for the k loop's and reduce_parts' signatures and holds nothing.)
template <bool N4>
__device__ __forceinline__ void pair_sums(const v16f (&acc)[2][2][kNQ], const v16f (&hh5)[2][2],
                                          int bi, int bj, int r, float parked, uint32_t *het_i,
                                          uint32_t *het_j, uint32_t *both_het, uint32_t *opp,
                                          uint32_t *hom_hom) {
  if constexpr (N4) {
    *het_i = (uint32_t)(2.f * acc[bi][bj][0][r]);
    *het_j = (uint32_t)(2.f * acc[bi][bj][1][r]);
    const uint32_t dd = (uint32_t)acc[bi][bj][2][r];
    const int32_t q = (int32_t)(0.25f * acc[bi][bj][3][r]);
    const uint32_t hh = (uint32_t)hh5[bi][bj][r];  // (full form only)
    *hom_hom = hh;
    *both_het = *het_i + *het_j - dd + hh;
    *opp = (uint32_t)((int32_t)hh - q) >> 1;
  } else {
    *het_i = (uint32_t)acc[bi][bj][2][r];
    *het_j = (uint32_t)acc[bi][bj][3][r];
    *both_het = (uint32_t)acc[bi][bj][1][r];
    *opp = (uint32_t)acc[bi][bj][0][r];
    *hom_hom = (uint32_t)parked;
  }
}

// Full form, records: sweep 0 decides every pair (cuking.cu:284-297) and
// counts, ONE reservation for the wavefront's records, sweep 1 stores them
// (cuking.cu:297-313; slot order inside the reservation: sweep order, then
// lane).  The decisions of sweep 0 are kept, one bit per pair.
// The fifth sum stays where the pass in front of the main loop parked it (five products:
// this lane's 16-byte slots `park`) and is read block by block.
// PIHAT (KIN = kPiHat): the same two sweeps with the PI_HAT decision and record
// (pihat_decide_call(), pihat_store_call(): TiledArgs::pihat instead of kin_threshold).
template <bool N4, bool PIHAT = false>
__device__ __forceinline__ void emit_full_records(const TiledArgs &a, const Segment &s,
                                                  const Lanes &l, const float4 *const park,
                                                  const v16f (&acc)[2][2][kNQ],
                                                  const v16f (&hh5)[2][2]) {
  const auto emit_ctx = emit_ctx_of<N4>(a);
  PihatArgs pihat = {};
  if constexpr (PIHAT) pihat = a.pihat;
  uint32_t total = 0, base = 0, run = 0;  // wave-uniform
  uint32_t decided[2 * 2] = {};           // bit r of word (bi, bj)
#pragma nounroll
  for (int pass = 0; pass < 2; ++pass) {  // (one body: the kernel has no registers for two)
#pragma unroll
    for (int bi = 0; bi < 2; ++bi) {
#pragma unroll
      for (int bj = 0; bj < 2; ++bj) {
        const uint32_t lj = pair_col(pair_origin(s, l), l, bj);
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          float hh[4] = {};
          if constexpr (!N4) unpack(park[park_slot(bi, bj, r4)], hh);
#pragma unroll
          for (int r1 = 0; r1 < 4; ++r1) {
            const int r = 4 * r4 + r1;
            const uint32_t li = pair_row(pair_origin(s, l), l, bi, r);
            uint32_t het_i, het_j, both_het, opp, hom_hom;
            pair_sums<N4>(acc, hh5, bi, bj, r, hh[r1], &het_i, &het_j, &both_het, &opp, &hom_hom);
            if (pass == 0) {
              bool emit = pair_valid(a, li, lj);
              if constexpr (PIHAT)
                emit = emit && pihat_decide_call(pihat, het_i, het_j, both_het, opp, hom_hom);
              else
                emit = emit && king_kinship(het_i, het_j, both_het, opp) > a.kin_threshold;
              decided[bi * 2 + bj] |= (emit ? 1u : 0u) << r;
            } else {
              const bool emit = (decided[bi * 2 + bj] >> r) & 1u;
              const unsigned long long b = __ballot(emit);
              if (b != 0) {  // wave-uniform
                const uint32_t before = __builtin_amdgcn_mbcnt_hi(
                    (uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
                const uint32_t slot = base + run + before;
                run += (uint32_t)__popcll(b);
                if constexpr (PIHAT) {
                  if (emit)
                    pihat_store_call(emit_ctx, pihat, slot, li, lj, het_i, het_j, both_het, opp,
                                     hom_hom);
                } else {
                  if (emit)
                    full_store_call(emit_ctx, slot, li, lj, het_i, het_j, both_het, opp, hom_hom);
                }
              }
            }
          }
        }
      }
    }
    if (pass == 0) {
      total = 0;
#pragma unroll
      for (int k = 0; k < 2 * 2; ++k) total += (uint32_t)__popc(decided[k]);
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) total += __shfl_xor(total, off);
      total = (uint32_t)__builtin_amdgcn_readfirstlane(total);
      if (total == 0) break;  // wave-uniform
      base = reserve_slots(a.result_index, total);
    }
  }
}

// Full form, diagnostic counts (TiledArgs::dense_counts): cuking.cu:284-313 with all five
// sums at hand, for every pair.
template <bool N4>
__device__ __forceinline__ void store_counts(const TiledArgs &a, const Segment &s, const Lanes &l,
                                             const float4 *const park,
                                             const v16f (&acc)[2][2][kNQ],
                                             const v16f (&hh5)[2][2]) {
#pragma unroll
  for (int bi = 0; bi < 2; ++bi) {
#pragma unroll
    for (int bj = 0; bj < 2; ++bj) {
      const uint32_t lj = pair_col(pair_origin(s, l), l, bj);
      float hh[16] = {};  // (five products) hom_hom of this block's 16 pairs
      if constexpr (!N4) {
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) unpack(park[park_slot(bi, bj, r4)], hh + 4 * r4);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const uint32_t li = pair_row(pair_origin(s, l), l, bi, r);
        uint32_t het_i, het_j, both_het, opp, hom_hom;
        pair_sums<N4>(acc, hh5, bi, bj, r, hh[r], &het_i, &het_j, &both_het, &opp, &hom_hom);
        full_epilogue_pair(a, pair_valid(a, li, lj), li, lj, het_i, het_j, both_het, opp, hom_hom);
      }
    }
  }
}

// Dense kinship (KIN): the lean epilogue's expression for every pair (four products:
// lean_epilogue_pair_n4's, on the exact integers hi, hj, num = hi + hj - 2 dd +
// 2 q), with the IEEE divide (pair_kin(), which the summary form shares) -- and one store.
// Column = lane & 31: the 32 lanes of a half-wave write 128 contiguous bytes of
// matrix row li.  (An unsorted layout: plane index = stored sample.)
// (kin_of_sums: from a pair's four accumulators s0 .. s3 -- the relative-counts form passes
//  them to its out-of-line epilogue)
template <bool N4>
__device__ __forceinline__ float kin_of_sums(float s0, float s1, float s2, float s3) {
  if constexpr (N4) {
    const uint32_t het_i = (uint32_t)(2.f * s0);
    const uint32_t het_j = (uint32_t)(2.f * s1);
    const int32_t num = (int32_t)(het_i + het_j) - 2 * (int32_t)s2 + 2 * (int32_t)(0.25f * s3);
    return 0.5f + (float)num / (4.f * (float)(het_i < het_j ? het_i : het_j));
  } else {
    // (five products: the accumulators are the reference's own four sums)
    return king_kinship((uint32_t)s2, (uint32_t)s3, (uint32_t)s1, (uint32_t)s0);
  }
}
template <bool N4>
__device__ __forceinline__ float pair_kin(const v16f (&acc)[2][2][kNQ], int bi, int bj, int r) {
  return kin_of_sums<N4>(acc[bi][bj][0][r], acc[bi][bj][1][r], acc[bi][bj][2][r], acc[bi][bj][3][r]);
}
template <bool N4>
__device__ __forceinline__ void store_kin(const TiledArgs &a, const Segment &s, const Lanes &l,
                                          const v16f (&acc)[2][2][kNQ]) {
  const PairOrigin o = pair_origin(s, l);
#pragma unroll
  for (int bi = 0; bi < 2; ++bi) {
#pragma unroll
    for (int bj = 0; bj < 2; ++bj) {
      const uint32_t lj = pair_col(o, l, bj);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const uint32_t li = pair_row(o, l, bi, r);
        // (symmetric output: the diagonal as well)
        const bool valid = pair_valid(a, li, lj, a.kin_diag);
        const float kin = pair_kin<N4>(acc, bi, bj, r);
        if (valid) a.dense_kin[(uint64_t)li * a.kin_ld + lj] = kin;
      }
    }
  }
}

// Kinship summary (KIN = summary): pair_kin() of every valid pair, REDUCED instead of stored.
// The tile's histogram (uint32: a tile has 16,384 pairs) and its 128 row + 128 column
// nearest-relative keys live in the LDS the stages no longer need: [row keys][column keys]
// [sum_bins + 3 counts].  A lane first reduces in registers what it holds -- the maximum over
// the two block columns of each of its 32 rows, the maximum over the 32 rows of each of its
// two columns -- then LDS atomics, then the workgroup adds the non-zero counts and raises the
// non-zero keys with one 64-bit global atomic each.  Slot and keys: king_kin_summary.h.
// Barriers on BOTH sides, whatever the mode: the phase zeroes LDS other wavefronts may still
// read operands from, and the next segment's LDS-DMA overwrites what it reads at its end.
// (The caller's vmcnt(0) comes first: every wavefront's own requests have landed.)
template <bool N4>
__device__ __forceinline__ void summarise_kin(const TiledArgs &a, const Segment &s, const Lanes &l,
                                              uint4 *const lds, const v16f (&acc)[2][2][kNQ]) {
  unsigned long long *const keys = reinterpret_cast<unsigned long long *>(lds);
  uint32_t *const hist = reinterpret_cast<uint32_t *>(keys + 2 * kTile);
  const bool want_hist = a.sum_hist != nullptr, want_best = a.sum_best != nullptr;  // uniform
  const uint32_t slots = want_hist ? kin_hist_slots(a.sum_bins) : 0u;
  __syncthreads();  // nobody reads the stages any more
  for (uint32_t k = threadIdx.x; k < 2 * kTile; k += 256) keys[k] = 0;
  for (uint32_t k = threadIdx.x; k < slots; k += 256) hist[k] = 0;
  __syncthreads();
  const PairOrigin o = pair_origin(s, l);
  unsigned long long col_key[2] = {0, 0};
#pragma unroll
  for (int bi = 0; bi < 2; ++bi) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const uint32_t li = pair_row(o, l, bi, r);
      unsigned long long row_key = 0;
#pragma unroll
      for (int bj = 0; bj < 2; ++bj) {
        const uint32_t lj = pair_col(o, l, bj);
        if (pair_valid(a, li, lj)) {
          const float kin = pair_kin<N4>(acc, bi, bj, r);
          if (want_hist) atomicAdd(&hist[kin_bin_slot(a.sum_lo, a.sum_scale, a.sum_bins, kin)], 1u);
          const unsigned long long kr = kin_best_key(kin, a.j_begin + lj);
          const unsigned long long kc = kin_best_key(kin, a.i_begin + li);
          row_key = kr > row_key ? kr : row_key;
          col_key[bj] = kc > col_key[bj] ? kc : col_key[bj];
        }
      }
      if (want_best && row_key != 0) atomicMax(&keys[l.wy * 64 + bi * 32 + c_row(r, l.g)], row_key);
    }
  }
#pragma unroll
  for (int bj = 0; bj < 2; ++bj)
    if (want_best && col_key[bj] != 0)
      atomicMax(&keys[kTile + l.wx * 64 + bj * 32 + l.lr], col_key[bj]);
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < slots; k += 256) {
    const uint32_t n = hist[k];
    if (n != 0) atomicAdd(&a.sum_hist[k], (unsigned long long)n);
  }
  if (want_best) {
    // thread t: row t of the tile, or column t - 128 (a non-zero key: a sample of the block)
    const uint32_t t = threadIdx.x, x = t & (kTile - 1);
    const unsigned long long key = keys[t];
    const uint32_t sample = t < kTile ? s.tr * kTile + x
                                      : (a.geo.diag ? 0u : a.geo.num_rows) + s.tc * kTile + x;
    if (key != 0) atomicMax(&a.sum_best[sample], key);
  }
  __syncthreads();  // the next segment's requests overwrite this
}

// Lean form, records.  Nearly every pair fails the threshold: decide that on the float
// sums without the IEEE divide, and only when some lane of the
// wavefront may pass run the exact epilogue (wave-uniform branch, out of line).
template <bool N4>
__device__ __forceinline__ void lean_decide(const TiledArgs &a, const Segment &s, const Lanes &l,
                                            const v16f (&acc)[2][2][kNQ]) {
  const PairOrigin o = pair_origin(s, l);
  const auto emit_ctx = emit_ctx_of<N4>(a);
#pragma unroll
  for (int bi = 0; bi < 2; ++bi) {
#pragma unroll
    for (int bj = 0; bj < 2; ++bj) {
      const uint32_t lj = pair_col(o, l, bj);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const uint32_t li = pair_row(o, l, bi, r);
        const bool valid = pair_valid(a, li, lj);
        if constexpr (N4) {
          // Four products: the decision needs hi, hj and the numerator
          // hi + hj - 2 dd + 2 q only; bh and opp of an emitted pair follow from
          // the recount of hom_hom (king_device.h).
          const float f_hi = 2.f * acc[bi][bj][0][r], f_hj = 2.f * acc[bi][bj][1][r];
          const float f_num = f_hi + f_hj - 2.f * acc[bi][bj][2][r] + 0.5f * acc[bi][bj][3][r];
          const bool maybe =
              valid && kinship_may_pass_num(f_num, fminf(f_hi, f_hj), a.kin_threshold);
          if (__ballot(maybe) != 0)
            lean_epilogue_call_n4(emit_ctx, valid, li, lj, (uint32_t)f_hi, (uint32_t)f_hj,
                                  (uint32_t)acc[bi][bj][2][r],
                                  (int32_t)(0.25f * acc[bi][bj][3][r]), l.lane);
        } else {
          const bool maybe =
              valid && kinship_may_pass(acc[bi][bj][2][r], acc[bi][bj][3][r],
                                        acc[bi][bj][1][r], acc[bi][bj][0][r], a.kin_threshold);
          if (__ballot(maybe) != 0)
            lean_epilogue_call(emit_ctx, valid, li, lj, (uint32_t)acc[bi][bj][2][r],
                               (uint32_t)acc[bi][bj][3][r], (uint32_t)acc[bi][bj][1][r],
                               (uint32_t)acc[bi][bj][0][r], l.lane);
        }
      }
    }
  }
}

// Relative counts (KIN = relative counts): lean_decide's cheap test against the lowest
// threshold (a.kin_threshold = rel_thr[0]), and only where some lane of the wavefront may pass
// the exact kinship, its band and the two atomics, out of line (rel_count_call()) -- no record
// and no hom_hom recount.  Pairs in plane order, like the records: each once.
template <bool N4>
__device__ __forceinline__ void count_relatives(const TiledArgs &a, const Segment &s,
                                                const Lanes &l, const v16f (&acc)[2][2][kNQ]) {
  const PairOrigin o = pair_origin(s, l);
  RelCtx c;
  c.counts = a.rel_counts;
  c.num = a.rel_num;
#pragma unroll
  for (uint32_t t = 0; t < CUKING_REL_THRESHOLDS_MAX; ++t) c.thr[t] = a.rel_thr[t];
  c.perm = a.perm;
  c.diag = a.geo.diag;
  c.num_rows = a.geo.num_rows;
  c.col_base = a.geo.col_base;
#pragma unroll
  for (int bi = 0; bi < 2; ++bi) {
#pragma unroll
    for (int bj = 0; bj < 2; ++bj) {
      const uint32_t lj = pair_col(o, l, bj);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const uint32_t li = pair_row(o, l, bi, r);
        const bool valid = pair_valid(a, li, lj);
        bool maybe;
        if constexpr (N4) {
          const float f_hi = 2.f * acc[bi][bj][0][r], f_hj = 2.f * acc[bi][bj][1][r];
          const float f_num = f_hi + f_hj - 2.f * acc[bi][bj][2][r] + 0.5f * acc[bi][bj][3][r];
          maybe = valid && kinship_may_pass_num(f_num, fminf(f_hi, f_hj), a.kin_threshold);
        } else {
          maybe = valid && kinship_may_pass(acc[bi][bj][2][r], acc[bi][bj][3][r],
                                            acc[bi][bj][1][r], acc[bi][bj][0][r], a.kin_threshold);
        }
        if (__ballot(maybe) != 0)
          rel_count_call<N4>(c, maybe, li, lj, acc[bi][bj][0][r], acc[bi][bj][1][r],
                             acc[bi][bj][2][r], acc[bi][bj][3][r]);
      }
    }
  }
}

// SPLIT = false: workgroup = one tile, all k-steps.
// SPLIT = true ("stream-k" remainder): the launch's tiles x k-steps are one
// line of work units cut into equal pieces, one per workgroup, so a remainder
// of tiles that would leave most CUs idle for a whole tile time still fills
// the chip.  A piece covers the end of one tile and/or the start of the next;
// each partial result (exact integers) is parked in a scratch slab, and the
// workgroup that delivers a tile's last part adds the others to its own and
// runs the epilogue.
// N4 = the four-product form on the nibble layout (four_product_loop()).
// KIN = kKinMatrix: the dense-kinship form of the lean kernels (TiledArgs::dense_kin): the same
// k loop, and an epilogue that stores the float32 kinship of EVERY pair instead of appending
// records; kKinSummary: the summary form (TiledArgs::sum_hist / sum_best), whose epilogue
// reduces that kinship instead (summarise_kin()) -- instantiations of their own, so that the epilogues of the others carry neither
// its branch nor its registers (a run-time branch in the shared full epilogue was enough
// for the five-product full form to reload a spilled value inside its k loop);
// kRelCounts: the relative-counts form (TiledArgs::rel_counts, count_relatives()), the lean
// record form without the records, which may run on a sorted layout like it.  The
// four-product one is the hot path; the five-product one serves contexts of variant 5 and
// bitsets from 2^22 sites on.
// The driver: take work -> per segment: hom_hom pass (FULL) -> k loop -> reduce parts
// (SPLIT, a partial tile) -> epilogue.
// kPiHat: the PI_HAT record form (TiledArgs::pihat), the only kind besides kRecords with FULL
// -- and with FULL only: the full form's two passes and an epilogue that decides on PI_HAT.
// (The kinds' values: king_launch_plan.h.)
template <bool FULL, bool SPLIT, bool N4 = false, int KIN = kRecords>
__global__ __launch_bounds__(256, 1) void king_mfma_kernel(const TiledArgs a) {
  static_assert(KIN == kRecords || (KIN == kPiHat ? FULL : !FULL),
                "the dense-kinship forms are lean ones, the PI_HAT form is a full one");
  extern __shared__ uint4 lds[];  // [NSTAGE][side][k-group][plane | slice][128]
  Work work;
  if (!take_work<SPLIT>(a, lds, &work)) return;  // uniform
  const Lanes l = lanes_of_thread();
  const NibbleMasks m = nibble_masks();
  uint32_t lane16 = l.lane * 16;  // (five_product_loop())
  Segment s;
  while (next_segment<SPLIT>(a, &work, &s)) {
    v16f hh5[2][2];  // full form: hom_hom of the wavefront's pairs (lean forms: never read)
    v16f acc[2][2][kNQ];
    if constexpr (FULL) hom_hom_pass<N4>(a, s, l, m, lds, hh5);
    if constexpr (N4) four_product_loop<FULL>(a, s, l, m, lds, acc, hh5);
    else five_product_loop<FULL>(a, s, l, m, lds, lane16, acc);
    // The clamped repeats of the last stage must have landed before the
    // workgroup's LDS goes away.
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    if (SPLIT) __syncthreads();  // ... and nobody reads the stages any more

    float4 *const park = FULL && !N4 ? park_slots(lds, l) : nullptr;
    if (SPLIT && s.num_steps != tile_steps_of(a) &&
        !reduce_parts<FULL, N4>(a, work.piece, s, l, lds, park, acc, hh5))
      continue;

    if constexpr (KIN == kPiHat) {
      emit_full_records<N4, true>(a, s, l, park, acc, hh5);
    } else if constexpr (FULL) {
      if (a.dense_counts == nullptr) emit_full_records<N4>(a, s, l, park, acc, hh5);
      else store_counts<N4>(a, s, l, park, acc, hh5);
    } else if constexpr (KIN == kKinMatrix) {
      store_kin<N4>(a, s, l, acc);
    } else if constexpr (KIN == kKinSummary) {
      summarise_kin<N4>(a, s, l, lds, acc);
    } else if constexpr (KIN == kRelCounts) {
      count_relatives<N4>(a, s, l, acc);
    } else {
      lean_decide<N4>(a, s, l, acc);
    }
    if (SPLIT) __syncthreads();  // LDS is reused by the next piece
  }
}

// The launch's shape (king_launch_plan.h) in the device arguments.
void set_shape(TiledArgs *a, const WholeShape &s) {
  a->launch_tiles = s.launch_tiles;
  a->xcd_chunk = s.xcd_chunk;
  a->dyn_tiles = s.dyn_tiles;
  a->dyn_wgs = s.dyn_wgs;
}

// Whole tiles [args.tile_begin, + num_blocks) in as many launches as the block limit asks
// for, or (SPLIT) the one launch of args.split_whole whole tiles + args.split_wgs pieces.
template <bool FULL, bool SPLIT, bool N4 = false, int KIN = kRecords>
hipError_t launch_shape(const TiledArgs &args, const LaunchSwitches &sw, uint64_t num_blocks,
                        uint32_t lds_bytes, hipStream_t stream) {
  constexpr auto kernel = king_mfma_kernel<FULL, SPLIT, N4, KIN>;
  // (five products: the caller's figure is the 6-stage one of the variant table)
  if (N4) lds_bytes = kMfmaN4LdsBytes;
  else if (FULL) lds_bytes += kMfmaParkBytes;  // the parked fifth sum, behind the stages
  else lds_bytes = kStagesPaired * kStageU4 * sizeof(uint4);
  hipError_t e = allow_dynamic_lds<kernel>(lds_bytes);
  if (e != hipSuccess) return e;
  TiledArgs a = args;
  if (SPLIT) {
    const WholeShape s = split_shape(args.split_whole, args.split_wgs, sw.xcd_swizzle);
    set_shape(&a, s);
    kernel<<<dim3((uint32_t)s.grid), dim3(256), lds_bytes, stream>>>(a);
    return hipGetLastError();
  }
  // (the dynamic tail's counter sits in the split scratch)
  const uint64_t dyn_min = args.split_counters != nullptr ? sw.dyn_tail_tiles : 0;
  const uint64_t cap = max_blocks_per_launch(256);
  for (uint64_t done = 0; done < num_blocks;) {
    const WholeShape s = whole_shape(num_blocks - done, cap, sw.xcd_swizzle, dyn_min, kMfmaDynFloor);
    a.tile_begin = args.tile_begin + done;
    set_shape(&a, s);
    kernel<<<dim3((uint32_t)s.grid), dim3(256), lds_bytes, stream>>>(a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    done += s.tiles;
  }
  return hipSuccess;
}

}  // namespace

size_t mfma_split_scratch_bytes(uint32_t wgs) {
  // one counter per tile (padded to 16 bytes), then two slabs of five sums per
  // workgroup
  return split_counter_bytes(wgs) + (size_t)wgs * 2 * (4 * 4 * 5 * 16 * 64) * sizeof(float);
}
size_t mfma_split_counter_bytes(uint32_t wgs) { return split_counter_bytes(wgs); }

namespace {
using Launch = hipError_t (*)(const TiledArgs &, const LaunchSwitches &, uint64_t, uint32_t,
                              hipStream_t);
// launch_shape<FULL, SPLIT, N4, KIN> by run-time flags, for the six kernel forms of
// kernel_form() (king_launch_plan.h): the records kind, which has both k loops, ...
constexpr Launch kRecordForms[2][2][2] = {  // [nibble][split][full]
    {{launch_shape<false, false, false>, launch_shape<true, false, false>},
     {launch_shape<false, true, false>, launch_shape<true, true, false>}},
    {{launch_shape<false, false, true>, launch_shape<true, false, true>},
     {launch_shape<false, true, true>, launch_shape<true, true, true>}}};
// ... and every other kind, which has one.
#define CUKING_KIND(FULL, KIN)                                                       \
  {{launch_shape<FULL, false, false, KIN>, launch_shape<FULL, true, false, KIN>},    \
   {launch_shape<FULL, false, true, KIN>, launch_shape<FULL, true, true, KIN>}}
constexpr Launch kKindForms[kNumKernelForms - 2][2][2] = {  // [kernel form - 2][nibble][split]
    CUKING_KIND(false, kKinMatrix), CUKING_KIND(false, kKinSummary),
    CUKING_KIND(false, kRelCounts), CUKING_KIND(true, kPiHat)};
#undef CUKING_KIND
static_assert(kKindForms[kNumKernelForms - 3][1][1] != nullptr, "a row for every kind");
Launch launch_of(int kernel_form, bool nibble, bool split) {
  return kernel_form < 2 ? kRecordForms[nibble][split][kernel_form]
                         : kKindForms[kernel_form - 2][nibble][split];
}

// What a form's kernels read of the device arguments, checked in front of any launch.
bool form_args_ok(CallForm form, const TiledArgs &a) {
  switch (form) {
    case kFormKinMatrix:  // (stored by position: an unsorted layout)
      return a.dense_kin != nullptr && a.perm == nullptr;
    case kFormKinSummary:
      // (the tile's histogram sits in LDS: kMfmaSummaryLdsBytes)
      return (a.sum_hist != nullptr || a.sum_best != nullptr) && a.perm == nullptr &&
             (a.sum_hist == nullptr || (a.sum_bins >= 1 && a.sum_bins <= CUKING_KIN_BINS_MAX));
    case kFormRelCounts:
      return a.rel_counts != nullptr && a.rel_num >= 1 && a.rel_num <= CUKING_REL_THRESHOLDS_MAX;
    case kFormPiHat:  // (records, and neither counts nor a matrix)
      return a.pihat.on != 0 && a.dense_counts == nullptr;
    default: return true;
  }
}

template <int KIN>
hipError_t launch_strided_form(const TiledArgs &a, uint32_t grid, hipStream_t stream) {
  constexpr auto kernel = king_mfma_kernel<false, false, true, KIN>;
  const hipError_t e = allow_dynamic_lds<kernel>(kMfmaN4LdsBytes);
  if (e != hipSuccess) return e;
  kernel<<<dim3(grid), dim3(256), kMfmaN4LdsBytes, stream>>>(a);
  return hipGetLastError();
}
// ONE launch of the four-product kernel's lean form with `grid` workgroups that stride over
// a list or a range, whatever the block limit (a test hook may set it below `grid`; a
// second launch would walk the list again).  Behind the filter kernel only: the forms its
// bound may apply to.
hipError_t launch_strided(CallForm form, const TiledArgs &a, uint32_t grid, hipStream_t stream) {
  if ((uint64_t)a.geo.k_words * 32 > kMfmaN4MaxSites || kernel_form(form, false) < 0 ||
      !kCallForms[form].filter_may_run || !form_args_ok(form, a))
    return hipErrorInvalidValue;
  const uint64_t cap = max_blocks_per_launch(256);
  if (grid > cap) grid = (uint32_t)cap;
  if (grid == 0) return hipErrorInvalidValue;
  return form == kFormRelCounts ? launch_strided_form<kRelCounts>(a, grid, stream)
                                : launch_strided_form<kRecords>(a, grid, stream);
}
}  // namespace

hipError_t launch_mfma_list(CallForm form, const TiledArgs &args, const uint2 *list,
                            const uint32_t *count, uint32_t cap, uint32_t grid,
                            hipStream_t stream) {
  if (list == nullptr) return hipErrorInvalidValue;
  TiledArgs a = args;
  a.tile_begin = 0;  // (the entries are tiles of the block, not of a range or a rectangle)
  a.rect_rows = 0;
  a.tile_list = list;
  a.tile_list_count = count;
  a.tile_list_cap = cap;
  return launch_strided(form, a, grid, stream);
}

hipError_t launch_mfma_gated(CallForm form, const TiledArgs &args, uint64_t num_units,
                             const uint32_t *gate, const uint8_t *skip_tiles, uint64_t skip_base,
                             uint32_t grid, hipStream_t stream) {
  if (gate == nullptr || num_units > 0xFFFFFFFFull) return hipErrorInvalidValue;
  TiledArgs a = args;
  a.gate = gate;
  a.gate_count = (uint32_t)num_units;
  a.skip_tiles = skip_tiles;
  a.skip_base = skip_base;
  return launch_strided(form, a, grid, stream);
}

hipError_t launch_mfma(bool full, bool nibble, const TiledArgs &args, const LaunchSwitches &sw,
                       uint64_t num_tiles, uint32_t lds_bytes, hipStream_t stream) {
  const int kf = kernel_form(sw.form, full);
  if (kf < 0 || !form_args_ok(sw.form, args) ||
      (uint64_t)args.geo.k_words * 32 > (nibble ? kMfmaN4MaxSites : kMfmaMaxSites))
    return hipErrorInvalidValue;
  // Whole tiles first, then ONE launch of whole tiles and the remainder in pieces
  // (king_launch_plan.h mfma_plan).  (Never split without scratch for the pieces.)
  const MfmaPlan p = mfma_plan(num_tiles, args.split_scratch != nullptr ? args.split_wgs : 0,
                               args.geo.k_words / 8, max_blocks_per_launch(256));
  hipError_t e = launch_of(kf, nibble, false)(args, sw, p.first, lds_bytes, stream);
  if (e != hipSuccess || p.split_tiles == 0) return e;
  TiledArgs a = args;
  a.tile_begin = args.tile_begin + p.first;
  a.split_whole = p.split_whole;
  a.split_tiles = p.split_tiles;
  return launch_of(kf, nibble, true)(a, sw, (uint64_t)p.split_whole + args.split_wgs, lds_bytes,
                                     stream);
}

// ---- symmetric fill of a dense kinship matrix --------------------------------------------
namespace {
constexpr uint32_t kMirrorTile = 32;
// Workgroup (bx, by), by <= bx, reads the 32 x 32 tile at rows 32 by, columns 32 bx of the
// upper triangle (rows of 128 contiguous bytes) into LDS and writes its transpose at rows
// 32 bx, columns 32 by (again rows of 128 bytes), strictly below the diagonal only.
__global__ __launch_bounds__(256) void kin_mirror_kernel(float *kin, const uint64_t ld,
                                                         const uint32_t n) {
  __shared__ float tile[kMirrorTile][kMirrorTile + 1];  // (+ 1: no bank conflicts on the columns)
  const uint32_t bx = blockIdx.x, by = blockIdx.y;
  if (by > bx) return;  // uniform
  const uint32_t x = threadIdx.x & 31, y0 = threadIdx.x >> 5;
#pragma unroll
  for (uint32_t y = y0; y < kMirrorTile; y += 8) {
    const uint32_t row = by * kMirrorTile + y, col = bx * kMirrorTile + x;
    if (row < n && col < n) tile[y][x] = kin[(uint64_t)row * ld + col];
  }
  __syncthreads();
#pragma unroll
  for (uint32_t y = y0; y < kMirrorTile; y += 8) {
    const uint32_t row = bx * kMirrorTile + y, col = by * kMirrorTile + x;
    if (row < n && col < row) kin[(uint64_t)row * ld + col] = tile[x][y];
  }
}
}  // namespace

hipError_t launch_kin_mirror(float *d_kin, uint64_t ld, uint32_t n, hipStream_t stream) {
  if (n < 2) return hipSuccess;
  const uint32_t tiles = (n + kMirrorTile - 1) / kMirrorTile;
  if (tiles > 65535) return hipErrorInvalidValue;  // (grid y; such a matrix is 16 TB)
  kin_mirror_kernel<<<dim3(tiles, tiles), dim3(256), 0, stream>>>(d_kin, ld, n);
  return hipGetLastError();
}

}  // namespace cuking
