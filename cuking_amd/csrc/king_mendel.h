// Mendelian errors of trios and duos (include/cuking_amd.h, "Mendelian errors"): the definitions
// the kernels of king_mendel.hip, the host twins of king_host.cc and the tests share, so that they
// cannot drift apart.  Plain C++: hipcc compiles the functions for the device, the sanitizer build
// of the tests (tests/mendel_host_driver.cc) for the host.  Integers only.
//
// Words are those of king_ibd.h: word w of a plane holds the sites 64 w .. 64 w + 63, and
// ibd_valid_mask(num_sites, w) the ones below num_sites.  Per sample and word the three called
// classes are disjoint masks (MendelWord); a sample that is absent -- a parent whose index is
// CUKING_MENDEL_NO_PARENT or >= num_stored -- is MendelWord{} (missing everywhere).  The eight
// code masks of a trio and word are pairwise disjoint, because the child's class and the pair of
// parental classes differ between any two rows of the table; their OR is the error mask.
#ifndef CUKING_AMD_KING_MENDEL_H_
#define CUKING_AMD_KING_MENDEL_H_

#include <cstdint>

#include "king_ibd.h"

namespace cuking {

constexpr uint32_t kMendelCodes = 8;
constexpr uint32_t kMendelNoParent = 0xFFFFFFFFu;  // CUKING_MENDEL_NO_PARENT

// One sample's word: hom-ref, het and hom-var among the valid sites; everything else is missing.
struct MendelWord {
  uint64_t ref = 0, het = 0, var = 0;
  CUKING_HD uint64_t called() const { return ref | het | var; }
};

CUKING_HD inline MendelWord mendel_word(uint64_t het, uint64_t hom, uint64_t valid) {
  MendelWord x;
  x.ref = ~het & ~hom & valid;
  x.het = het & ~hom & valid;
  x.var = hom & ~het & valid;
  return x;
}

// code[k]: the sites with error code k + 1 (the numbers of PLINK and Hail, autosomal).  "not V" and
// "not R" of a parent include missing and absent, which is what makes a duo work.
CUKING_HD inline void mendel_code_masks(const MendelWord &f, const MendelWord &m,
                                        const MendelWord &c, uint64_t code[kMendelCodes]) {
  code[0] = f.ref & m.ref & c.het;
  code[1] = f.var & m.var & c.het;
  code[2] = f.var & ~m.var & c.ref;
  code[3] = ~f.var & m.var & c.ref;
  code[4] = f.var & m.var & c.ref;
  code[5] = f.ref & ~m.ref & c.var;
  code[6] = ~f.ref & m.ref & c.var;
  code[7] = f.ref & m.ref & c.var;
}

// The sites counted as `called`: the child's and those of every parent that is not NO_PARENT (a
// listed parent >= num_stored is missing everywhere: nothing is called).
CUKING_HD inline uint64_t mendel_called(const MendelWord &f, bool has_f, const MendelWord &m,
                                        bool has_m, const MendelWord &c) {
  return c.called() & (has_f ? f.called() : ~0ull) & (has_m ? m.called() : ~0ull);
}

}  // namespace cuking

#endif  // CUKING_AMD_KING_MENDEL_H_
