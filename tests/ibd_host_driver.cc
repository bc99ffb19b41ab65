// Stand-alone driver of the host side of the IBD segments for the sanitizer build of
// tests/test_ibd_host.py (built and run by tests/host_driver.py, csrc/king_host.cc linked in).
// Every buffer is an exact-size heap allocation, so a byte read or written past an end is caught
// -- the planes of exactly ceil(num_sites / 64) words above all: the word of bit num_sites lies
// beyond them when num_sites is a multiple of 64.
//   1. cuking_ibd_pairs_host against a walk over the sites one by one, for shapes around the
//      word and step edges, with and without groups and positions, both strides: the rows, the
//      segment count, the segment set; buffers of exactly the count, of one less
//      (RESOURCE_EXHAUSTED, the exact count) and the counting call with a null buffer;
//   2. the refusals, a decreasing position, the calls without work.
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

void run_shape(uint32_t n, uint32_t sites, bool groups, bool positions, uint32_t stride,
               uint32_t min_sites) {
  const uint32_t plane = sites ? (sites + 63) / 64 : 1, words = 2 * plane;
  std::unique_ptr<uint64_t[]> bits(new uint64_t[(size_t)n * words]);
  // sparse breaks: mostly hom-ref / het, few hom-var, some missing; long runs exist
  for (size_t k = 0; k < (size_t)n * words; ++k) {
    const bool hom = (k / plane) & 1;
    bits[k] = hom ? next_random() & next_random() & next_random() & next_random() & next_random()
                  : next_random() & next_random();
  }
  // sample 1 copies sample 0 over the middle half
  for (uint32_t s = sites / 4; s < sites - sites / 4; ++s)
    for (uint32_t p = 0; p < 2; ++p) {
      const uint64_t bit = 1ull << (s & 63);
      uint64_t &to = bits[words + p * plane + (s >> 6)];
      to = (to & ~bit) | (bits[p * plane + (s >> 6)] & bit);
    }
  std::unique_ptr<int32_t[]> group(new int32_t[sites]);
  std::unique_ptr<uint32_t[]> pos(new uint32_t[sites]);
  for (uint32_t s = 0; s < sites; ++s) {
    group[s] = (int32_t)(s / 200) - (s >= 64 ? 5 : 0);
    // (a new group may start anywhere; without groups the positions never decrease)
    const bool first = s == 0 || (groups && group[s] != group[s - 1]);
    pos[s] = first ? (uint32_t)(next_random() % 100) : pos[s - 1] + (uint32_t)(next_random() % 4);
  }
  const int32_t *g = groups && sites ? group.get() : nullptr;
  const uint32_t *q = positions && sites ? pos.get() : nullptr;
  std::vector<std::pair<uint32_t, uint32_t>> list;
  for (uint32_t i = 0; i < n; ++i)
    for (uint32_t j = i; j < n; ++j) list.push_back({i, j});
  list.push_back({1, 0});
  list.push_back({n, 0});
  list.push_back({0, 0xFFFFFFFFu});
  const uint64_t num_pairs = list.size();
  std::unique_ptr<unsigned char[]> pairs(new unsigned char[num_pairs * stride]);
  memset(pairs.get(), 0xEE, num_pairs * stride);
  for (uint64_t p = 0; p < num_pairs; ++p) {
    const uint32_t in[2] = {list[p].first, list[p].second};
    memcpy(pairs.get() + p * stride, in, 8);
  }

  // the walk over the sites
  std::vector<cuking_ibd_pair> want(num_pairs);
  std::vector<Seg> want_segs;
  const uint32_t min_length = positions ? 40 : 0;
  for (uint64_t p = 0; p < num_pairs; ++p) {
    cuking_ibd_pair row = {list[p].first, list[p].second, 0, 0, 0, 0, 0, 0};
    if (row.sample_i < n && row.sample_j < n) {
      const uint64_t *ri = bits.get() + (size_t)row.sample_i * words;
      const uint64_t *rj = bits.get() + (size_t)row.sample_j * words;
      for (uint32_t kind = 1; kind <= 2; ++kind) {
        int64_t first = -1;
        uint32_t count = 0, longest = 0;
        uint64_t total = 0;
        auto close = [&](uint32_t last) {
          const uint32_t a = (uint32_t)first, len = q ? q[last] - q[a] : last - a;
          if (last - a + 1 >= min_sites && len >= min_length) {
            ++count;
            total += len;
            longest = std::max(longest, len);
            want_segs.push_back(Seg((uint32_t)p, kind, a, last));
          }
          first = -1;
        };
        for (uint32_t s = 0; s < sites; ++s) {
          if (first >= 0 && g && g[s] != g[s - 1]) close(s - 1);
          const uint32_t ci = code_of(ri, plane, s), cj = code_of(rj, plane, s);
          const bool called = ci != 3 && cj != 3;
          const bool brk = called && (kind == 1 ? ci + cj == 2 && ci != 1 : ci != cj);
          if (brk) {
            if (first >= 0) close(s - 1);
          } else if (first < 0) {
            first = s;
          }
        }
        if (first >= 0) close(sites - 1);
        (kind == 1 ? row.segments1 : row.segments2) = count;
        (kind == 1 ? row.length1 : row.length2) = total;
        (kind == 1 ? row.longest1 : row.longest2) = longest;
      }
    }
    want[p] = row;
  }
  std::sort(want_segs.begin(), want_segs.end());
  const uint64_t total = want_segs.size();

  for (int mode = 0; mode < 4; ++mode) {
    // 0: no list; 1: exactly the count; 2: one less; 3: the counting call
    if (mode == 2 && total == 0) continue;
    const uint64_t room = mode == 1 ? total : mode == 2 ? total - 1 : 0;
    std::unique_ptr<cuking_ibd_pair[]> out(new cuking_ibd_pair[num_pairs]);
    std::unique_ptr<cuking_ibd_segment[]> segs(new cuking_ibd_segment[room]);
    uint64_t found = 12345;
    const cuking_status st = cuking_ibd_pairs_host(
        bits.get(), n, words, sites, g, q, min_sites, min_length, pairs.get(), num_pairs, stride,
        out.get(), room ? segs.get() : nullptr, room, mode == 0 ? nullptr : &found);
    const bool overflow = mode != 0 && total > room;
    if (st != (overflow ? CUKING_ERR_RESOURCE_EXHAUSTED : CUKING_OK))
      return fail("status", sites, (uint64_t)st * 10 + mode);
    if (mode != 0 && found != total) return fail("count", sites, found);
    if (memcmp(out.get(), want.data(), num_pairs * sizeof(cuking_ibd_pair)) != 0)
      return fail("rows", sites, mode);
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
  std::unique_ptr<uint32_t[]> pos(new uint32_t[sites]);
  std::unique_ptr<int32_t[]> group(new int32_t[sites]);
  for (uint32_t s = 0; s < sites; ++s) {
    pos[s] = 10 * s;
    group[s] = s >= 70;
  }
  const uint32_t pairs[2] = {0, 1};
  cuking_ibd_pair out;
  cuking_ibd_segment seg;
  uint64_t found = 0;
  const cuking_status bad = CUKING_ERR_INVALID_ARGUMENT;
#define CALL(...) cuking_ibd_pairs_host(__VA_ARGS__)
  expect("ok", CALL(bits.get(), 2, words, sites, group.get(), pos.get(), 64, 0, pairs, 1, 8, &out,
                    &seg, 1, &found), CUKING_ERR_RESOURCE_EXHAUSTED);  // one segment of each kind
  if (found != 2 || out.segments1 != 1 || out.segments2 != 1 || out.length1 != 690)
    fail("two groups of 70 and 58 sites", sites, found);
  expect("odd words", CALL(bits.get(), 2, 3, sites, nullptr, nullptr, 64, 0, pairs, 1, 8, &out,
                           nullptr, 0, nullptr), bad);
  expect("zero words", CALL(bits.get(), 2, 0, 0, nullptr, nullptr, 64, 0, pairs, 1, 8, &out,
                            nullptr, 0, nullptr), bad);
  expect("too many sites", CALL(bits.get(), 2, words, 129, nullptr, nullptr, 64, 0, pairs, 1, 8,
                                &out, nullptr, 0, nullptr), bad);
  expect("min_sites", CALL(bits.get(), 2, words, sites, nullptr, nullptr, 63, 0, pairs, 1, 8,
                           &out, nullptr, 0, nullptr), bad);
  expect("stride", CALL(bits.get(), 2, words, sites, nullptr, nullptr, 64, 0, pairs, 1, 6, &out,
                        nullptr, 0, nullptr), bad);
  expect("null out", CALL(bits.get(), 2, words, sites, nullptr, nullptr, 64, 0, pairs, 1, 8,
                          nullptr, nullptr, 0, nullptr), bad);
  expect("null pairs", CALL(bits.get(), 2, words, sites, nullptr, nullptr, 64, 0, nullptr, 1, 8,
                            &out, nullptr, 0, nullptr), bad);
  expect("null bits", CALL(nullptr, 2, words, sites, nullptr, nullptr, 64, 0, pairs, 1, 8, &out,
                           nullptr, 0, nullptr), bad);
  expect("segments without a counter", CALL(bits.get(), 2, words, sites, nullptr, nullptr, 64, 0,
                                            pairs, 1, 8, &out, &seg, 1, nullptr), bad);
  expect("null segments", CALL(bits.get(), 2, words, sites, nullptr, nullptr, 64, 0, pairs, 1, 8,
                               &out, nullptr, 1, &found), bad);
  pos[100] = 5;
  expect("decreasing pos", CALL(bits.get(), 2, words, sites, group.get(), pos.get(), 64, 0, pairs,
                                1, 8, &out, nullptr, 0, nullptr), CUKING_ERR_FAILED_PRECONDITION);
  pos[100] = 1000;
  pos[70] = 0;  // (the first site of a group may lie below its predecessor)
  expect("a new group restarts", CALL(bits.get(), 2, words, sites, group.get(), pos.get(), 64, 0,
                                      pairs, 1, 8, &out, nullptr, 0, nullptr), CUKING_OK);
  expect("no pairs", CALL(nullptr, 0, words, sites, nullptr, nullptr, 64, 0, nullptr, 0, 8,
                          nullptr, nullptr, 0, &found), CUKING_OK);
  expect("no sites", CALL(nullptr, 2, words, 0, nullptr, nullptr, 64, 0, pairs, 1, 8, &out,
                          nullptr, 0, &found), CUKING_OK);
  if (out.sample_j != 1 || out.segments1 != 0 || out.length1 != 0) fail("zero row", 0, 0);
#undef CALL
}

}  // namespace

int main() {
  const uint32_t shapes[] = {1, 63, 64, 65, 127, 128, 129, 640, 4095, 4096, 4097, 8192 + 37};
  int k = 0;
  for (uint32_t sites : shapes)
    for (int variant = 0; variant < 4; ++variant, ++k)
      run_shape(3, sites, variant & 1, variant & 2, k % 3 == 0 ? 24 : 8, k % 2 ? 64 : 100);
  run_refusals();
  printf("%d failures\n", g_failures);
  return g_failures != 0;
}
