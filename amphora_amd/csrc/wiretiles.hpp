// Tile ownership of the segmented wire-text kernels (k_rv_b64_seg /
// k_mask_b64_seg): which object and which of its tiles a workgroup decodes.
// Shared by the kernels, the host-side validation of the slotted layout and
// the CPU tests, so it compiles for the host alone (as seglookup.hpp).
//
// word_offsets[n_objects + 1]: offsets[0] = 0, nondecreasing, offsets[n_objects]
// = T; object o holds W_o = offsets[o + 1] - offsets[o] words and is decoded in
// ceil(W_o / t) tiles of t words (t = 192: one 256-lane workgroup's 4,096
// characters of every field).
//
// With g(o) = offsets[o] / t + o (integer division), g is strictly increasing
// and g(o + 1) - g(o) >= ceil(W_o / t):
//   offsets[o + 1] / t >= floor((offsets[o] + W_o) / t) >= offsets[o] / t +
//   floor(W_o / t), and the "+ o" adds one more, which covers the partial tile.
// So workgroup w of a grid of T / t + n_objects (> g(n_objects - 1) +
// ceil(W_last / t) - 1) owns local tile w - g(o) of the LAST o with g(o) <= w,
// when that tile exists (t (w - g(o)) < W_o), and nothing otherwise: every
// real tile has exactly one owner, no scan and no scratch.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "seglookup.hpp"

namespace amph {

constexpr size_t kWireTileWords = 192;  // Wire<kWireBlock>::words (wire.hip asserts it)

// characters of the base64 text of `words` 16-byte words, '=' padding included
AMPH_SEG_HD inline size_t wire_text_chars(size_t words) { return 4 * ((16 * words + 2) / 3); }
// the dense slotted layout's stride: the text rounded up to whole 16-byte units
AMPH_SEG_HD inline size_t wire_slot_chars(size_t words) { return (wire_text_chars(words) + 15) & ~(size_t)15; }

// The MaskedInput "data" array text of `words` records (37 bytes each, the
// trailing ',' / ']' included, after one '['; "[]" for none) and its stride in
// the dense 16-byte-aligned layout (include/amphora_upload_batch.h).  The
// segmented K_CONV (k_conv_json_seg) applies the ownership rule below at
// t = kConvTileWords, one workgroup's records; an object of no words has no
// tile there but still a text, "[]", which workgroup g(o) handles: it exists
// (g(o) < T / t + n_objects) and, g being strictly increasing with
// g(o + 1) >= g(o) + 1, it is no other object's real tile.
constexpr size_t kConvTileWords = 128;  // kPairBlock (kernels.hip asserts it)
AMPH_SEG_HD inline size_t masked_input_data_chars(size_t words) { return words ? 37 * words + 1 : 2; }
AMPH_SEG_HD inline size_t upload_slot_chars(size_t words) {
  return (masked_input_data_chars(words) + 15) & ~(size_t)15;
}

// workgroups of the launch over T words in n_objects objects
AMPH_SEG_HD inline size_t wire_tile_grid(uint64_t total_words, size_t n_objects, size_t t = kWireTileWords) {
  return (size_t)(total_words / t) + n_objects;
}

struct WireTile {
  size_t object;  // in [0, n_objects) whatever the table holds
  size_t local;   // tile of that object; real iff wire_tile_real(local, W_object)
};
// (compared in tiles, not words: a broken table's local may be near 2^64)
AMPH_SEG_HD inline bool wire_tile_real(size_t local, uint64_t object_words, size_t t = kWireTileWords) {
  return local < (object_words + t - 1) / t;
}

// The tile of workgroup w.  Bisection over [0, n_objects) as seg_find:
// bounded by n_objects, offsets[n_objects] is never read here, and the object
// lies in range for any table (n_objects >= 1) -- a table that breaks the
// contract misplaces tiles, it cannot index outside the verdict arrays.
AMPH_SEG_HD inline WireTile wire_tile_find(const uint64_t* offsets, size_t n_objects, uint64_t w,
                                           size_t t = kWireTileWords) {
  size_t lo = 0, hi = n_objects;
  while (hi - lo > 1) {
    const size_t mid = lo + (hi - lo) / 2;
    if (offsets[mid] / t + mid <= w) lo = mid;
    else hi = mid;
  }
  const uint64_t g = offsets[lo] / t + lo;
  return WireTile{lo, (size_t)(w - g)};  // w < g only for a broken table: a huge local, no tile
}

}  // namespace amph
