// Object lookup of the packed (segmented) calls: which object of an offsets
// table owns a word.  Shared by the kernels' failure path, the host-side
// gather of amph_*_batch and the CPU tests, so it compiles for the host alone.
//
// offsets[n_objects + 1] are word offsets: offsets[0] = 0, nondecreasing,
// offsets[n_objects] = T; object o owns [offsets[o], offsets[o + 1]).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AMPH_SEG_HD __host__ __device__
#else
#define AMPH_SEG_HD
#endif

namespace amph {

// The object that owns word i < T: the LAST o with offsets[o] <= i, so the
// empty objects that share a start with their successor are passed over.
// Bisection over [0, n_objects): offsets[n_objects] is never read and the
// result lies in [0, n_objects) whatever the table holds (n_objects >= 1) --
// a table that breaks the contract misplaces a verdict, it cannot index
// outside the verdict array.
AMPH_SEG_HD inline size_t seg_find(const uint64_t* offsets, size_t n_objects, uint64_t i) {
  size_t lo = 0, hi = n_objects;
  while (hi - lo > 1) {
    const size_t mid = lo + (hi - lo) / 2;
    if (offsets[mid] <= i) lo = mid;
    else hi = mid;
  }
  return lo;
}

}  // namespace amph
