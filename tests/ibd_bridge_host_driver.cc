// Stand-alone driver of the host side of the IBD segments with bridged breaks for the sanitizer
// build of tests/test_ibd_bridge_host.py (built and run by tests/host_driver.py, csrc/king_host.cc
// linked in).  Every buffer is an exact-size heap allocation, so a byte read or written past an
// end is caught -- the group-start mask read for a link and the planes of exactly
// ceil(num_sites / 64) words above all.
//   1. cuking_ibd_pairs_bridged_host against a walk over the sites one by one that links its
//      runs afterwards: sample 1 copies sample 0 but for single opposite homozygotes at the word
//      and step edges, next to each other, next to a group boundary, at site 0 and at the last
//      site, and close to the end (a chain that is pending when the scan ends); sample 2 is
//      random.  Rows, bridged counts, the segment count and set; a null `bridged`; buffers of
//      exactly the count and of one less; bridge_sites 0 against cuking_ibd_pairs_host;
//   2. the refusals bridge_sites = 1 and 63, and a refusal of the strict call.
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

void run_shape(uint32_t sites, bool groups, bool positions, uint32_t stride, uint32_t min_sites,
               uint32_t bridge_sites) {
  const uint32_t n = 3, plane = (sites + 63) / 64, words = 2 * plane;
  std::unique_ptr<uint64_t[]> bits(new uint64_t[(size_t)n * words]);
  for (size_t k = 0; k < (size_t)n * words; ++k) bits[k] = next_random() & next_random();
  // sample 1 is sample 0, then single opposite homozygotes
  memcpy(bits.get() + words, bits.get(), words * sizeof(uint64_t));
  // (319 and 4095: bit 63 of a word and of a step; 448 and 4416: bit 0; 150, 151: neighbours)
  const uint32_t breaks[] = {0,    150,  151,  319,  448,         700,        799,      1000,
                             1100, 4095, 4300, 4416, sites - 130, sites - 65, sites - 1};
  for (uint32_t s : breaks)
    if (s < sites) {
      set_code(bits.get(), plane, s, 0);
      set_code(bits.get() + words, plane, s, 2);
    }
  std::unique_ptr<int32_t[]> group(new int32_t[sites]);
  std::unique_ptr<uint32_t[]> pos(new uint32_t[sites]);
  for (uint32_t s = 0; s < sites; ++s) {
    // groups start at 800 (behind the break at 799), 1000 (at a break), 1600, ...
    group[s] = s < 800 ? 3 : s < 1000 ? 9 : (int32_t)(s / 1600) - 4;
    const bool first = s == 0 || (groups && group[s] != group[s - 1]);
    pos[s] = first ? (uint32_t)(next_random() % 100) : pos[s - 1] + (uint32_t)(next_random() % 4);
  }
  const int32_t *g = groups ? group.get() : nullptr;
  const uint32_t *q = positions ? pos.get() : nullptr;
  const uint32_t list[][2] = {{0, 1}, {1, 0}, {0, 2}, {1, 1}, {n, 0}, {0, 0xFFFFFFFFu}, {1, 2}};
  const uint64_t num_pairs = sizeof(list) / sizeof(list[0]);
  std::unique_ptr<unsigned char[]> pairs(new unsigned char[num_pairs * stride]);
  memset(pairs.get(), 0xEE, num_pairs * stride);
  for (uint64_t p = 0; p < num_pairs; ++p) memcpy(pairs.get() + p * stride, list[p], 8);

  // the walk over the sites, then the links
  std::vector<cuking_ibd_pair> want(num_pairs);
  std::vector<uint32_t> want_bridged(2 * num_pairs, 0);
  std::vector<Seg> want_segs;
  const uint32_t min_length = positions ? 40 : 0;
  for (uint64_t p = 0; p < num_pairs; ++p) {
    cuking_ibd_pair row = {list[p][0], list[p][1], 0, 0, 0, 0, 0, 0};
    if (row.sample_i < n && row.sample_j < n) {
      const uint64_t *ri = bits.get() + (size_t)row.sample_i * words;
      const uint64_t *rj = bits.get() + (size_t)row.sample_j * words;
      for (uint32_t kind = 1; kind <= 2; ++kind) {
        std::vector<Run> runs;
        int64_t first = -1;
        for (uint32_t s = 0; s < sites; ++s) {
          if (first >= 0 && g && g[s] != g[s - 1]) {
            runs.push_back({(uint32_t)first, s - 1});
            first = -1;
          }
          const uint32_t ci = code_of(ri, plane, s), cj = code_of(rj, plane, s);
          const bool called = ci != 3 && cj != 3;
          const bool brk = called && (kind == 1 ? ci + cj == 2 && ci != 1 : ci != cj);
          if (brk) {
            if (first >= 0) runs.push_back({(uint32_t)first, s - 1});
            first = -1;
          } else if (first < 0) {
            first = s;
          }
        }
        if (first >= 0) runs.push_back({(uint32_t)first, sites - 1});
        uint32_t count = 0, longest = 0, forgiven = 0;
        uint64_t total = 0;
        for (size_t k = 0; k < runs.size();) {
          size_t end = k;  // the chain runs[k .. end]
          while (end + 1 < runs.size() && bridge_sites != 0) {
            const Run &l = runs[end], &r = runs[end + 1];
            const bool one_group = !g || (g[l.b] == g[l.b + 1] && g[l.b + 1] == g[r.a]);
            if (r.a != l.b + 2 || !one_group || l.b - l.a + 1 < bridge_sites ||
                r.b - r.a + 1 < bridge_sites)
              break;
            ++end;
          }
          const uint32_t a = runs[k].a, b = runs[end].b, len = q ? q[b] - q[a] : b - a;
          if (b - a + 1 >= min_sites && len >= min_length) {
            ++count;
            total += len;
            longest = std::max(longest, len);
            forgiven += (uint32_t)(end - k);
            want_segs.push_back(Seg((uint32_t)p, kind, a, b));
          }
          k = end + 1;
        }
        (kind == 1 ? row.segments1 : row.segments2) = count;
        (kind == 1 ? row.length1 : row.length2) = total;
        (kind == 1 ? row.longest1 : row.longest2) = longest;
        want_bridged[2 * p + kind - 1] = forgiven;
      }
    }
    want[p] = row;
  }
  std::sort(want_segs.begin(), want_segs.end());
  const uint64_t total = want_segs.size();
  if (bridge_sites != 0 && sites >= 640 && want_bridged[0] == 0)
    fail("nothing was bridged", sites, bridge_sites);

  for (int mode = 0; mode < 4; ++mode) {
    // 0: no list, null bridged; 1: exactly the count; 2: one less; 3: the counting call
    if (mode == 2 && total == 0) continue;
    const uint64_t room = mode == 1 ? total : mode == 2 ? total - 1 : 0;
    std::unique_ptr<cuking_ibd_pair[]> out(new cuking_ibd_pair[num_pairs]);
    std::unique_ptr<uint32_t[]> bridged(new uint32_t[2 * num_pairs]);
    std::unique_ptr<cuking_ibd_segment[]> segs(new cuking_ibd_segment[room]);
    uint64_t found = 12345;
    const cuking_status st = cuking_ibd_pairs_bridged_host(
        bits.get(), n, words, sites, g, q, min_sites, min_length, bridge_sites, pairs.get(),
        num_pairs, stride, out.get(), mode == 0 ? nullptr : bridged.get(),
        room ? segs.get() : nullptr, room, mode == 0 ? nullptr : &found);
    const bool overflow = mode != 0 && total > room;
    if (st != (overflow ? CUKING_ERR_RESOURCE_EXHAUSTED : CUKING_OK))
      return fail("status", sites, (uint64_t)st * 10 + mode);
    if (mode != 0 && found != total) return fail("count", sites, found);
    if (memcmp(out.get(), want.data(), num_pairs * sizeof(cuking_ibd_pair)) != 0)
      return fail("rows", sites, mode);
    if (mode != 0 && memcmp(bridged.get(), want_bridged.data(), 8 * num_pairs) != 0)
      return fail("bridged", sites, mode);
    if (mode == 1) {
      std::vector<Seg> got;
      for (uint64_t k = 0; k < total; ++k)
        got.push_back(Seg(segs[k].pair, segs[k].kind, segs[k].first_site, segs[k].last_site));
      std::sort(got.begin(), got.end());
      if (got != want_segs) return fail("segments", sites, total);
      if (bridge_sites == 0) {  // the strict call: the same rows and the same list
        std::unique_ptr<cuking_ibd_segment[]> other(new cuking_ibd_segment[room]);
        if (cuking_ibd_pairs_host(bits.get(), n, words, sites, g, q, min_sites, min_length,
                                  pairs.get(), num_pairs, stride, out.get(),
                                  room ? other.get() : nullptr, room, &found) != CUKING_OK ||
            found != total || memcmp(out.get(), want.data(), num_pairs * 40) != 0 ||
            memcmp(other.get(), segs.get(), room * sizeof(cuking_ibd_segment)) != 0)
          return fail("the strict call", sites, found);
      }
    }
  }
}

void run_refusals() {
  const uint32_t sites = 128, words = 4;
  std::unique_ptr<uint64_t[]> bits(new uint64_t[2 * words]());
  const uint32_t pairs[2] = {0, 1};
  cuking_ibd_pair out;
  uint32_t bridged[2] = {7, 7};
  const cuking_status bad = CUKING_ERR_INVALID_ARGUMENT;
  for (uint32_t bridge : {1u, 63u})
    expect("bridge_sites", cuking_ibd_pairs_bridged_host(bits.get(), 2, words, sites, nullptr,
                                                         nullptr, 64, 0, bridge, pairs, 1, 8,
                                                         &out, bridged, nullptr, 0, nullptr), bad);
  expect("min_sites", cuking_ibd_pairs_bridged_host(bits.get(), 2, words, sites, nullptr, nullptr,
                                                    63, 0, 64, pairs, 1, 8, &out, bridged,
                                                    nullptr, 0, nullptr), bad);
  if (bridged[0] != 7 || bridged[1] != 7) fail("a refused call wrote", sites, bridged[0]);
  for (uint32_t bridge : {0u, 64u, 0xFFFFFFFFu})
    expect("ok", cuking_ibd_pairs_bridged_host(bits.get(), 2, words, sites, nullptr, nullptr, 64,
                                               0, bridge, pairs, 1, 8, &out, bridged, nullptr, 0,
                                               nullptr), CUKING_OK);
  if (out.segments1 != 1 || out.length2 != 127 || bridged[0] != 0) fail("one run", sites, 0);
}

}  // namespace

int main() {
  const uint32_t shapes[] = {640, 4096, 4097, 8192 + 37};
  int k = 0;
  for (uint32_t sites : shapes)
    for (int variant = 0; variant < 4; ++variant)
      for (uint32_t bridge : {0u, 64u, 100u}) {
        run_shape(sites, variant & 1, variant & 2, k % 3 == 0 ? 24 : 8, k % 2 ? 150 : 200, bridge);
        ++k;
      }
  run_refusals();
  printf("%d failures\n", g_failures);
  return g_failures != 0;
}
