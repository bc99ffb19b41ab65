// Stand-alone driver of the host side of the runs of homozygosity for the sanitizer build of
// tests/test_roh_host.py (built and run by tests/host_driver.py, csrc/king_host.cc linked in).
// Every buffer is an exact-size heap allocation, so a byte read or written past an end is caught
// -- the planes of exactly ceil(num_sites / 64) words, the group-start mask read for a link and
// the list of samples above all.
//   1. cuking_roh_samples_host against a walk over the sites one by one that links its runs
//      afterwards: sample 0 is homozygous but for single hets at the word and step edges, next to
//      each other, next to a group boundary, at site 0 and at the last site, and close to the end
//      (a chain that is pending when the scan ends); sample 1 is random, sample 2 wholly missing.
//      Rows, the segment count and set; the null list; buffers of exactly the count and of one
//      less; the counting call;
//   2. the refusals bridge_sites = 1 and 63 and min_sites = 63, which write nothing.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <tuple>
#include <vector>

#include "cuking_amd.h"
#include "host_driver_common.h"

namespace {

typedef std::tuple<uint32_t, uint32_t, uint32_t, uint32_t> Seg;
struct Run {
  uint32_t a, b;
};

void run_shape(uint32_t sites, bool groups, bool positions, bool listed, uint32_t min_sites,
               uint32_t bridge_sites) {
  const uint32_t n = 3, plane = (sites + 63) / 64, words = 2 * plane;
  std::unique_ptr<uint64_t[]> bits(new uint64_t[(size_t)n * words]);
  for (size_t k = 0; k < (size_t)n * words; ++k) bits[k] = next_random();
  // sample 0: hom-ref or hom-var or (rarely) missing, then single hets; the padding stays random
  for (uint32_t s = 0; s < sites; ++s) {
    const uint32_t code = code_of(bits.get(), plane, s);
    set_code(bits.get(), plane, s, code == 1 ? (next_random() % 50 ? 2 : 3) : code);
  }
  // (319 and 4095: bit 63 of a word and of a step; 448 and 4416: bit 0; 150, 151: neighbours)
  const uint32_t hets[] = {0,    150,  151,  319,  448,         700,        799,      1000,
                           1100, 4095, 4300, 4416, sites - 130, sites - 65, sites - 1};
  for (uint32_t s : hets)
    if (s < sites) set_code(bits.get(), plane, s, 1);
  // sample 2: wholly missing
  for (uint32_t s = 0; s < sites; ++s) set_code(bits.get() + 2 * words, plane, s, 3);
  std::unique_ptr<int32_t[]> group(new int32_t[sites]);
  std::unique_ptr<uint32_t[]> pos(new uint32_t[sites]);
  for (uint32_t s = 0; s < sites; ++s) {
    // groups start at 800 (behind the het at 799), 1000 (at a het), 1600, ...
    group[s] = s < 800 ? 3 : s < 1000 ? 9 : (int32_t)(s / 1600) - 4;
    const bool first = s == 0 || (groups && group[s] != group[s - 1]);
    pos[s] = first ? (uint32_t)(next_random() % 100) : pos[s - 1] + (uint32_t)(next_random() % 4);
  }
  const int32_t *g = groups ? group.get() : nullptr;
  const uint32_t *q = positions ? pos.get() : nullptr;
  const uint32_t list[] = {0, 2, 1, 0, n, 0xFFFFFFFFu, 2};
  const uint64_t num_samples = listed ? sizeof(list) / sizeof(list[0]) : n;
  std::unique_ptr<uint32_t[]> samples(new uint32_t[num_samples]);
  for (uint64_t r = 0; r < num_samples; ++r) samples[r] = listed ? list[r] : (uint32_t)r;

  // the walk over the sites, then the links
  std::vector<cuking_roh_sample> want(num_samples);
  std::vector<Seg> want_segs;
  const uint32_t min_length = positions ? 40 : 0;
  for (uint64_t r = 0; r < num_samples; ++r) {
    cuking_roh_sample row;
    memset(&row, 0, sizeof(row));
    row.sample = samples[r];
    if (row.sample < n) {
      const uint64_t *mine = bits.get() + (size_t)row.sample * words;
      std::vector<Run> runs;
      int64_t first = -1;
      for (uint32_t s = 0; s < sites; ++s) {
        if (first >= 0 && g && g[s] != g[s - 1]) {
          runs.push_back({(uint32_t)first, s - 1});
          first = -1;
        }
        if (code_of(mine, plane, s) == 1) {
          if (first >= 0) runs.push_back({(uint32_t)first, s - 1});
          first = -1;
        } else if (first < 0) {
          first = s;
        }
      }
      if (first >= 0) runs.push_back({(uint32_t)first, sites - 1});
      for (size_t k = 0; k < runs.size();) {
        size_t end = k;  // the chain runs[k .. end]
        while (end + 1 < runs.size() && bridge_sites != 0) {
          const Run &l = runs[end], &rr = runs[end + 1];
          const bool one_group = !g || (g[l.b] == g[l.b + 1] && g[l.b + 1] == g[rr.a]);
          if (rr.a != l.b + 2 || !one_group || l.b - l.a + 1 < bridge_sites ||
              rr.b - rr.a + 1 < bridge_sites)
            break;
          ++end;
        }
        const uint32_t a = runs[k].a, b = runs[end].b, len = q ? q[b] - q[a] : b - a;
        if (b - a + 1 >= min_sites && len >= min_length) {
          ++row.segments;
          row.length += len;
          row.longest = std::max(row.longest, len);
          row.bridged += (uint32_t)(end - k);
          want_segs.push_back(Seg((uint32_t)r, CUKING_ROH_KIND, a, b));
        }
        k = end + 1;
      }
    }
    want[r] = row;
  }
  std::sort(want_segs.begin(), want_segs.end());
  const uint64_t total = want_segs.size();
  if (bridge_sites != 0 && sites >= 640 && want[0].bridged == 0)
    fail("nothing was bridged", sites, bridge_sites);
  if (sites >= 640 && total == 0) fail("no segment", sites, bridge_sites);

  for (int mode = 0; mode < 4; ++mode) {
    // 0: no list of segments; 1: exactly the count; 2: one less; 3: the counting call
    if (mode == 2 && total == 0) continue;
    const uint64_t room = mode == 1 ? total : mode == 2 ? total - 1 : 0;
    std::unique_ptr<cuking_roh_sample[]> out(new cuking_roh_sample[num_samples]);
    memset(out.get(), 0xEE, num_samples * sizeof(cuking_roh_sample));
    std::unique_ptr<cuking_ibd_segment[]> segs(new cuking_ibd_segment[room]);
    uint64_t found = 12345;
    const cuking_status st = cuking_roh_samples_host(
        bits.get(), n, words, sites, g, q, min_sites, min_length, bridge_sites,
        listed ? samples.get() : nullptr, num_samples, out.get(), room ? segs.get() : nullptr,
        room, mode == 0 ? nullptr : &found);
    const bool overflow = mode != 0 && total > room;
    if (st != (overflow ? CUKING_ERR_RESOURCE_EXHAUSTED : CUKING_OK))
      return fail("status", sites, (uint64_t)st * 10 + mode);
    if (mode != 0 && found != total) return fail("count", sites, found);
    for (uint64_t r = 0; r < num_samples; ++r)
      if (out[r].length != want[r].length || out[r].sample != want[r].sample ||
          out[r].segments != want[r].segments || out[r].longest != want[r].longest ||
          out[r].bridged != want[r].bridged)
        return fail("rows", sites, r * 10 + mode);
    if (mode == 1) {
      std::vector<Seg> got;
      for (uint64_t k = 0; k < total; ++k)
        got.push_back(Seg(segs[k].pair, segs[k].kind, segs[k].first_site, segs[k].last_site));
      std::sort(got.begin(), got.end());
      if (got != want_segs) return fail("segments", sites, total);
    }
  }
}

void run_refusals() {
  const uint32_t sites = 128, words = 4;
  std::unique_ptr<uint64_t[]> bits(new uint64_t[2 * words]());
  cuking_roh_sample out[2];
  memset(out, 0x77, sizeof(out));
  const cuking_status bad = CUKING_ERR_INVALID_ARGUMENT;
  for (uint32_t bridge : {1u, 63u})
    expect("bridge_sites", cuking_roh_samples_host(bits.get(), 2, words, sites, nullptr, nullptr,
                                                   64, 0, bridge, nullptr, 2, out, nullptr, 0,
                                                   nullptr), bad);
  expect("min_sites", cuking_roh_samples_host(bits.get(), 2, words, sites, nullptr, nullptr, 63,
                                              0, 64, nullptr, 2, out, nullptr, 0, nullptr), bad);
  if (out[0].segments != 0x77777777u || out[1].length != 0x7777777777777777ull)
    fail("a refused call wrote", sites, out[0].segments);
  for (uint32_t bridge : {0u, 64u, 0xFFFFFFFFu})
    expect("ok", cuking_roh_samples_host(bits.get(), 2, words, sites, nullptr, nullptr, 64, 0,
                                         bridge, nullptr, 2, out, nullptr, 0, nullptr), CUKING_OK);
  // all hom-ref: one run over all 128 sites
  if (out[0].segments != 1 || out[1].length != 127 || out[1].sample != 1 || out[0].bridged != 0)
    fail("one run", sites, 0);
}

}  // namespace

int main() {
  const uint32_t shapes[] = {640, 4096, 4097, 8192 + 37};
  int k = 0;
  for (uint32_t sites : shapes)
    for (int variant = 0; variant < 4; ++variant)
      for (uint32_t bridge : {0u, 64u, 100u}) {
        run_shape(sites, variant & 1, variant & 2, k % 3 != 0, k % 2 ? 150 : 200, bridge);
        ++k;
      }
  run_refusals();
  printf("%d failures\n", g_failures);
  return g_failures != 0;
}
