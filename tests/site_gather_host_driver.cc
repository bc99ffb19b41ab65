// Stand-alone driver of the byte-wide site gather's arithmetic (csrc/king_site_gather.h) for the
// sanitizer build of tests/test_site_gather_host.py (built and run by tests/host_driver.py, with
// nothing of the library linked in: of host_driver_common.h it uses what calls none of it).
// gather_sites_kernel (csrc/king_sort.hip) replayed on the host, lane by lane, with the header's
// helpers -- interleave, nibble pack, field lookup, 8 x 8 transposes, byte routing --, for G = 2
// and G = 4, against a plain bit loop.  The staged sites and the wavefront's tile are exact-size
// heap allocations, so a byte read or written past an end is caught.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <numeric>
#include <vector>

#include "host_driver_common.h"
#include "king_site_gather.h"

namespace {

using namespace cuking;

constexpr uint64_t kUnwritten = 0xA5A5A5A5A5A5A5A5ull;

// out[s][plane] bit d = bits[s][plane] bit order[d]
std::vector<uint64_t> plain(const std::vector<uint64_t> &bits, uint32_t n, uint32_t wps,
                            const std::vector<uint32_t> &order) {
  const uint32_t P = wps / 2;
  std::vector<uint64_t> out((size_t)n * wps, kUnwritten);
  for (uint32_t s = 0; s < n; ++s)
    for (uint32_t plane = 0; plane < 2; ++plane) {
      const uint64_t *src = &bits[(size_t)s * wps + plane * P];
      uint64_t *dst = &out[(size_t)s * wps + plane * P];
      for (uint32_t w = 0; w < P; ++w) dst[w] = 0;
      for (uint32_t d = 0; d < 64 * P; ++d) {
        const uint32_t at = order[d];
        dst[d >> 6] |= ((src[at >> 6] >> (at & 63)) & 1ull) << (d & 63);
      }
    }
  return out;
}

// One workgroup of gather_sites_kernel<G>, its wavefronts one after the other.
void replay_group(uint32_t G, const std::vector<uint64_t> &bits, uint32_t n, uint32_t wps,
                  const std::vector<uint32_t> &order, uint32_t s0, std::vector<uint64_t> *out) {
  const uint32_t P = wps / 2;
  std::unique_ptr<uint8_t[]> site(new uint8_t[gather_site_bytes(G, P)]);
  for (uint32_t w = 0; w < P; ++w) {
    uint64_t f[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t g = 0; g < G; ++g) {
      const uint32_t s = s0 + g < n ? s0 + g : n - 1;
      f[gather_field_bit(g, 0)] = bits[(size_t)s * wps + w];
      f[gather_field_bit(g, 1)] = bits[(size_t)s * wps + P + w];
    }
    for (uint32_t b = 0; b < 8; ++b) {
      const uint64_t x = gather_interleave8(f, b);
      if (G == 4) {
        memcpy(&site[64 * w + 8 * b], &x, 8);
      } else {
        const uint32_t y = gather_pack_nibbles(x);
        memcpy(&site[32 * w + 4 * b], &y, 4);
      }
    }
  }
  std::unique_ptr<uint8_t[]> tile(new uint8_t[kGatherTileBytes]);
  for (uint32_t w0 = 0; w0 < P; w0 += kGatherBatch) {
    for (uint32_t lane = 0; lane < 64; ++lane)
      for (uint32_t k = 0; k < kGatherBatch; ++k) {
        const uint32_t W = w0 + k < P ? w0 + k : P - 1;
        const uint32_t src = order[64 * W + lane];
        tile[64 * k + lane] = (uint8_t)gather_field_of(G, src, site[gather_byte_index(G, src)]);
      }
    uint64_t x[kGatherBatch / 8][64];
    for (uint32_t r = 0; r < kGatherBatch / 8; ++r)
      for (uint32_t lane = 0; lane < 64; ++lane) memcpy(&x[r][lane], &tile[8 * (64 * r + lane)], 8);
    for (uint32_t r = 0; r < kGatherBatch / 8; ++r)
      for (uint32_t lane = 0; lane < 64; ++lane) {
        const uint64_t y = gather_assemble8(x[r][lane]);
        const uint32_t k = 8 * r + (lane >> 3), b = lane & 7;
        for (uint32_t f = 0; f < 2 * G; ++f) tile[gather_out_byte(f, k, b)] = (uint8_t)(y >> (8 * f));
      }
    for (uint32_t i = 0; i < 2 * G * kGatherBatch; ++i) {
      const uint32_t f = gather_out_field(i), k = gather_out_word(i), s = s0 + f / 2;
      uint64_t word;
      memcpy(&word, &tile[8 * i], 8);
      if (w0 + k < P && s < n) (*out)[(size_t)s * wps + (f & 1) * P + w0 + k] = word;
    }
  }
}

std::vector<uint32_t> make_order(int kind, uint32_t sites) {
  std::vector<uint32_t> order(sites);
  std::iota(order.begin(), order.end(), 0u);
  if (kind == 1) std::reverse(order.begin(), order.end());
  if (kind == 2)
    for (uint32_t i = sites - 1; i > 0; --i) std::swap(order[i], order[next_random() % (i + 1)]);
  if (kind == 3) {  // a stable descending sort of weights with many ties
    std::vector<uint32_t> weight(sites);
    for (uint32_t &w : weight) w = (uint32_t)(next_random() % 5);
    std::stable_sort(order.begin(), order.end(),
                     [&](uint32_t a, uint32_t b) { return weight[a] > weight[b]; });
  }
  return order;
}

void check_transpose() {
  for (int round = 0; round < 64; ++round) {
    const uint64_t x = round == 0 ? 0x8040201008040201ull : next_random();
    const uint64_t y = transpose8x8(x);
    for (uint32_t r = 0; r < 8; ++r)
      for (uint32_t c = 0; c < 8; ++c)
        if (((x >> (8 * r + c)) & 1) != ((y >> (8 * c + r)) & 1)) {
          fprintf(stderr, "transpose8x8: bit (%u, %u) of %016llx\n", r, c, (unsigned long long)x);
          ++g_failures;
          return;
        }
  }
}

}  // namespace

int main() {
  check_transpose();
  const uint32_t samples[] = {1, 2, 3, 5, 9};
  // (words per sample: the planes of 1, 3, 7, 65 and 320 words, and one with a word behind them)
  const uint32_t widths[] = {2, 6, 14, 130, 640, 15};
  int cases = 0;
  for (uint32_t n : samples)
    for (uint32_t wps : widths) {
      const uint32_t P = wps / 2;
      std::vector<uint64_t> bits((size_t)n * wps);
      for (uint64_t &w : bits) w = next_random();
      for (int kind = 0; kind < 4; ++kind) {
        const std::vector<uint32_t> order = make_order(kind, 64 * P);
        const std::vector<uint64_t> want = plain(bits, n, wps, order);
        for (uint32_t G : {2u, 4u}) {
          std::vector<uint64_t> got((size_t)n * wps, kUnwritten);
          for (uint32_t s0 = 0; s0 < n; s0 += G) replay_group(G, bits, n, wps, order, s0, &got);
          ++cases;
          if (got != want) {
            fprintf(stderr, "G = %u: %u samples x %u words per sample, order %d\n", G, n, wps, kind);
            ++g_failures;
          }
        }
      }
    }
  printf("%d cases, %d failures\n", cases, g_failures);
  return g_failures != 0;
}
