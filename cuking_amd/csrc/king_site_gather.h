// The arithmetic of the byte-wide site gather (king_sort.hip, gather_sites_kernel), as code
// shared by host, device and tests (tests/site_gather_host_driver.cc replays it against a
// plain bit loop).
//
// A workgroup stages G samples in LDS interleaved PER SITE: site s owns one field of 2 G
// bits, bit 2 g + plane of it the bit of sample g in plane `plane` (0 het, 1 hom-alt) --
// a byte per site for G = 4, a nibble for G = 2 (even site low, odd site high).  A lane that
// reads the field of order[d] then holds destination site d of all G samples and both
// planes, and 64 lanes x 2 G bits become 2 G output words by transposing 8 x 8 bit
// matrices, not by voting.
#ifndef CUKING_KING_SITE_GATHER_H_
#define CUKING_KING_SITE_GATHER_H_

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CUKING_GATHER_HD __host__ __device__ __forceinline__
#else
#define CUKING_GATHER_HD inline
#endif

namespace cuking {

// Destination words a wavefront assembles at a time: lane l of a gather round holds site l of
// one of them, and a (sample, plane) row leaves as 8 kGatherBatch contiguous bytes.
constexpr uint32_t kGatherBatch = 16;
// LDS behind the staged sites, per wavefront: kGatherBatch words x 64 sites, a byte each.
constexpr uint32_t kGatherTileBytes = kGatherBatch * 64;

// The bit of sample g (< G) and plane (0 het, 1 hom-alt) within a site's field.
CUKING_GATHER_HD uint32_t gather_field_bit(uint32_t g, uint32_t plane) { return 2 * g + plane; }

// Bytes of LDS the staged sites of `plane_words` words per plane take.
CUKING_GATHER_HD uint32_t gather_site_bytes(uint32_t group, uint32_t plane_words) {
  return group == 4 ? 64 * plane_words : 32 * plane_words;
}

// 8 x 8 bit matrix, row r in byte r: bit c of byte r <-> bit r of byte c (three delta swaps).
CUKING_GATHER_HD uint64_t transpose8x8(uint64_t x) {
  uint64_t t = (x ^ (x >> 7)) & 0x00AA00AA00AA00AAull;
  x ^= t ^ (t << 7);
  t = (x ^ (x >> 14)) & 0x0000CCCC0000CCCCull;
  x ^= t ^ (t << 14);
  t = (x ^ (x >> 28)) & 0x00000000F0F0F0F0ull;
  x ^= t ^ (t << 28);
  return x;
}

// Staging.  `fields[f]`: the source word (64 sites) of field bit f, f < 2 G, zero behind
// them.  The eight sites 8 b .. 8 b + 7 of the word as eight bytes, site 8 b + i in byte i,
// its field in the byte's low 2 G bits.
CUKING_GATHER_HD uint64_t gather_interleave8(const uint64_t fields[8], uint32_t b) {
  uint64_t x = 0;
#pragma unroll
  for (uint32_t f = 0; f < 8; ++f) x |= ((fields[f] >> (8 * b)) & 0xFFull) << (8 * f);
  return transpose8x8(x);
}

// G = 2: eight bytes of gather_interleave8 (fields in the low nibbles) as four, even site
// in the low nibble of its byte, odd site in the high one.
CUKING_GATHER_HD uint32_t gather_pack_nibbles(uint64_t x) {
  x = (x | (x >> 4)) & 0x00FF00FF00FF00FFull;
  x = (x | (x >> 8)) & 0x0000FFFF0000FFFFull;
  return (uint32_t)(x | (x >> 16));
}

// The field of stored site `src` out of the staged bytes (`at(byte index)` reads one).
CUKING_GATHER_HD uint32_t gather_byte_index(uint32_t group, uint32_t src) {
  return group == 4 ? src : src >> 1;
}
CUKING_GATHER_HD uint32_t gather_field_of(uint32_t group, uint32_t src, uint32_t byte) {
  return group == 4 ? byte : (byte >> (4 * (src & 1))) & 0xFu;
}

// Assembly.  The fields of destination sites 8 b .. 8 b + 7 of one word, site 8 b + i in
// byte i: byte f of the result is byte b of that word for field bit f.
CUKING_GATHER_HD uint64_t gather_assemble8(uint64_t fields_of_sites) {
  return transpose8x8(fields_of_sites);
}
// Where that byte goes in a wavefront's tile of finished words, [field bit][word of the
// batch][byte], ...
CUKING_GATHER_HD uint32_t gather_out_byte(uint32_t f, uint32_t k, uint32_t b) {
  return (f * kGatherBatch + k) * 8 + b;
}
// ... and which (field bit, word of the batch) the 64-bit word at index i of that tile is.
CUKING_GATHER_HD uint32_t gather_out_field(uint32_t i) { return i / kGatherBatch; }
CUKING_GATHER_HD uint32_t gather_out_word(uint32_t i) { return i % kGatherBatch; }

}  // namespace cuking

#endif  // CUKING_KING_SITE_GATHER_H_
