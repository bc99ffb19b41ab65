// Prints the launch plans of csrc/king_launch_plan.h for a grid of inputs
// (tests/test_launch_plan.py compares the output with tests/golden/launch_plans.txt): a
// readable selection one line per input, then the whole grid as one FNV-1a hash of its lines
// per kernel, workgroup count and block limit ("--all" prints those lines instead).
//
//   m <tiles> <wgs> <cap> <steps> <xcd> <dyn> | launches of the four-/five-product kernel:
//       w <begin> <tiles> <shape>                     whole-tile launch
//       s <begin> <split_whole> <split_tiles> <shape> whole tiles + remainder pieces
//   f <tiles> <wgs> <cap> <steps> <switch set> | launch chunks of the filter kernel:
//       c <n> <check0> <check1> <rotate> <rest> <parts> <shape> <fsplit_tile0> <fsplit_first> <grid>
//   "--mfma <tiles> <wgs> <cap> <steps> ..." prints mfma_plan alone for the inputs given
//   (tests/pihat_fuzz_cases.py asks which calls of a sweep launch remainder pieces).
//   <shape> = <launch_tiles> <xcd_chunk> <dyn_tiles> <dyn_wgs> <grid>; launch_tiles prints as
//   "-" where no kernel reads it (plain order, no dynamic tail).
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "king_launch_plan.h"

using namespace cuking;

static std::string g_line;  // the line being built
static void out(const char *fmt, ...) {
  char buf[256];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_line += buf;
}

static const uint64_t kHwBlocks = 0xFFFFFFFFull / 256;  // workgroups of 256 threads per launch
static const uint64_t kChunkTiles = 1u << 17;           // kFilterChunkTiles
static const uint32_t kSlabs = 256;                     // kFilterSplitSlabs

static void print_shape(const WholeShape &s) {
  if (s.xcd_chunk == 0 && s.dyn_tiles == 0) out(" -");
  else out(" %u", s.launch_tiles);
  out(" %u %u %u %llu", s.xcd_chunk, s.dyn_tiles, s.dyn_wgs, (unsigned long long)s.grid);
}

// launch_mfma + launch_shape (king_mfma.hip) with the launches printed
static void plan_mfma(uint64_t tiles, uint32_t wgs, uint64_t cap, uint32_t steps, uint32_t xcd,
                      uint32_t dyn) {
  const MfmaPlan p = mfma_plan(tiles, wgs, steps, cap);
  // (the dynamic tail's counter sits in the split scratch: none without it)
  for (uint64_t done = 0; done < p.first;) {
    const WholeShape s = whole_shape(p.first - done, cap, xcd, wgs != 0 ? dyn : 0, kMfmaDynFloor);
    out(" w %llu %llu", (unsigned long long)done, (unsigned long long)s.tiles);
    print_shape(s);
    done += s.tiles;
  }
  if (p.split_tiles != 0) {
    out(" s %llu %u %u", (unsigned long long)p.first, p.split_whole, p.split_tiles);
    print_shape(split_shape(p.split_whole, wgs, xcd));
  }
}

struct FilterCase {
  const char *name;
  bool checks;
  LaunchSwitches sw;
};

// launch_filter (king_filter.hip) with the chunks printed
static void plan_filter(uint64_t tiles, uint32_t split_wgs, uint64_t cap, uint32_t steps,
                        const FilterCase &c) {
  if (cap > kChunkTiles) cap = kChunkTiles;
  const uint32_t wgs = split_wgs != 0 ? split_wgs : 256;
  for (uint64_t done = 0; done < tiles;) {
    const FilterPlan p =
        filter_plan(tiles - done, cap, wgs, steps, c.checks, split_wgs != 0, kSlabs, c.sw);
    out(" c %llu %u %u %u %u %u", (unsigned long long)p.n, p.check0, p.check1, p.rotate,
           p.rest, p.parts);
    print_shape(p.whole);
    out(" %u %u %llu", p.fsplit_tile0, p.fsplit_first, (unsigned long long)p.grid);
    done += p.n;
  }
}

// ---- the grid of inputs ----

static const uint32_t kWgs[] = {0, 256, 304};
static const uint64_t kCaps[] = {0, 64, 300, 1000};  // 0 = the hardware limit only
static const uint32_t kSteps[] = {7, 64, 391};
static const uint32_t kMfmaSwitches[][2] = {{2, 16384}, {1, 16384}, {0, 16384}, {2, 0}};
// xcd_swizzle, dyn_tail_tiles, check0, check1, check_emit, rotate, rotate_min_tiles,
// split_min_steps, filter_runs
static const FilterCase kFilterCases[] = {
    {"default", true, {2, 16384, 1, 1, 64, 1, 2048, 8, true}},
    {"off", false, {0, 0, 0, 0, 0, 0, 0, 0, true}},
    {"forced", true, {1, 16384, 2, 3, 255, 2, 2048, 1, true}},
    {"other", true, {2, 1024, 1, 9, 0, 1, 0, 64, true}},
};
// Tile counts around every threshold of the planners, and the benchmark configurations':
// configs[1] 820 (256-sample tiles) / 3,160 (128), configs[2] 76,636 / 306,153, configs[3]
// 687,378 / 2,748,340, configs[4] 4,114,146 / 16,447,980.
static const uint64_t kCounts[] = {
    1,     7,     36,    63,    64,     65,     255,    256,    257,     287,     288,     289,
    300,   511,   512,   513,   607,    608,    609,    767,    768,     820,     1023,    1024,
    1216,  2047,  2048,  2049,  3160,   4095,   4096,   4097,   4864,    16383,   16384,   16385,
    19455, 19456, 65536, 76636, 131072, 131073, 306153, 687378, 2748340, 4114146, 16447980};
static const uint64_t kKeyCounts[] = {36, 300, 820, 3160, 4096, 19456, 76636, 306153};
static const uint32_t kDense = 4200;  // hashed part: every count up to this one as well

static bool g_print = true;  // print the lines, or hash them
static uint64_t g_hash, g_lines;
static void end_line() {
  if (g_print) {
    puts(g_line.c_str());
  } else {
    g_line += '\n';
    for (unsigned char c : g_line) g_hash = (g_hash ^ c) * 0x100000001B3ull;
    ++g_lines;
  }
  g_line.clear();
}
static void mfma_line(uint64_t t, uint32_t wgs, uint64_t cap, uint32_t steps, const uint32_t *sw) {
  out("m %llu %u %llu %u %u %u |", (unsigned long long)t, wgs, (unsigned long long)cap, steps,
      sw[0], sw[1]);
  plan_mfma(t, wgs, cap != 0 ? cap : kHwBlocks, steps, sw[0], sw[1]);
  end_line();
}
static void filter_line(uint64_t t, uint32_t wgs, uint64_t cap, uint32_t steps,
                        const FilterCase &c) {
  out("f %llu %u %llu %u %s |", (unsigned long long)t, wgs, (unsigned long long)cap, steps,
      c.name);
  plan_filter(t, wgs, cap != 0 ? cap : kHwBlocks, steps, c);
  end_line();
}
static void both(uint64_t t, uint32_t wgs, uint64_t cap, uint32_t steps, int sw) {
  mfma_line(t, wgs, cap, steps, kMfmaSwitches[sw]);
  if (t > 8 * kChunkTiles) return;  // (many chunks: in the hashed part only)
  filter_line(t, wgs, cap, steps, kFilterCases[sw]);
}

// "--forms": the rules of the call forms (kCallForms), one line per form:
//   <form index> <name> | <k loop> <unsorted> <filter_may_run> <valu_serves> | lean <kernel>
//   full <kernel>        <kernel> = <KIN> <FULL> <kernel_form()>, or "refused"
static int print_forms() {
  static const char *const kLoops[] = {"either", "full", "lean"};
  for (int f = 0; f < kNumCallForms; ++f) {
    const CallFormRules &r = kCallForms[f];
    printf("%d %s | %s %d %d %d |", f, r.name, kLoops[r.k_loop], r.unsorted, r.filter_may_run,
           r.valu_serves);
    for (int full = 0; full < 2; ++full) {
      const int kf = kernel_form((CallForm)f, full != 0);
      if (kf < 0) printf(" %s refused", full ? "full" : "lean");
      else printf(" %s %d %d %d", full ? "full" : "lean", r.kin, full, kf);
    }
    printf("\n");
  }
  // (a form outside the table is refused, not read)
  printf("outside %d %d\n", kernel_form((CallForm)-1, false), kernel_form(kNumCallForms, true));
  return 0;
}

// "--mfma <tiles> <wgs> <cap> <steps> ...": mfma_plan for each group of four numbers (cap 0 =
// the hardware limit only), one line per group: <first> <split_whole> <split_tiles>
static int print_mfma(int count, char **words) {
  if (count % 4 != 0) return 2;
  for (int k = 0; k < count; k += 4) {
    const uint64_t tiles = strtoull(words[k], nullptr, 10), cap = strtoull(words[k + 2], nullptr, 10);
    const uint32_t wgs = (uint32_t)strtoul(words[k + 1], nullptr, 10);
    const uint32_t steps = (uint32_t)strtoul(words[k + 3], nullptr, 10);
    const MfmaPlan p = mfma_plan(tiles, wgs, steps, cap != 0 ? cap : kHwBlocks);
    printf("%llu %u %u\n", (unsigned long long)p.first, p.split_whole, p.split_tiles);
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc > 1 && strcmp(argv[1], "--forms") == 0) return print_forms();
  if (argc > 1 && strcmp(argv[1], "--mfma") == 0) return print_mfma(argc - 2, argv + 2);
  const bool all = argc > 1 && strcmp(argv[1], "--all") == 0;
  // Readable part: every count at the defaults (256 CUs, no block limit, 100k sites), then a
  // few counts with one input changed at a time (a block limit: lines of at most 16 launches).
  for (uint64_t t : kCounts) both(t, 256, 0, 391, 0);
  for (uint64_t t : kKeyCounts) {
    for (uint32_t wgs : {0u, 304u}) both(t, wgs, 0, 391, 0);
    for (uint32_t steps : {7u, 64u}) both(t, 256, 0, steps, 0);
    for (uint64_t cap : {64u, 300u, 1000u})
      if (t <= 16 * cap) both(t, 256, cap, 391, 0);
    for (int sw = 1; sw < 4; ++sw) both(t, 256, 0, 391, sw);
  }
  // Hashed part: the full cross of counts (1 .. kDense and kCounts), k-steps and switch sets
  // per kernel, workgroup count and block limit.
  g_print = all;
  for (int filter = 0; filter < 2; ++filter)
    for (uint32_t wgs : kWgs)
      for (uint64_t cap : kCaps) {
        g_hash = 0xCBF29CE484222325ull;
        g_lines = 0;
        for (size_t k = 0; k < kDense + sizeof kCounts / sizeof *kCounts; ++k) {
          const uint64_t t = k < kDense ? k + 1 : kCounts[k - kDense];
          // (a block limit is a test hook of small runs: no line of more than 256 launches)
          if (cap != 0 && t > 256 * cap) continue;
          for (uint32_t steps : kSteps)
            for (int sw = 0; sw < 4; ++sw) {
              if (filter) filter_line(t, wgs, cap, steps, kFilterCases[sw]);
              else mfma_line(t, wgs, cap, steps, kMfmaSwitches[sw]);
            }
        }
        if (!all)
          printf("hash %c %u %llu | %llu lines %016llx\n", filter ? 'f' : 'm', wgs,
                 (unsigned long long)cap, (unsigned long long)g_lines, (unsigned long long)g_hash);
      }
  return 0;
}
