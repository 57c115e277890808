// Geometry of the segmented exchange codec (k_xencs_* / k_xdecs_*,
// exchange.hip; include/amphora_exchange_batch.h): which object's pairs an
// encode workgroup formats, and which object's text a decode workgroup parses.
// Shared by the kernels, the host-side table checks and the CPU tests, so it
// compiles for the host alone (as wiretiles.hpp / respondtiles.hpp).
//
// ENCODE.  pair_offsets[n_objects + 1]: 0 first, nondecreasing, npairs_total
// last; object o holds P_o pairs and is written by max(1, ceil(P_o / 256))
// tiles of 256 pairs -- an object of no pairs keeps the one tile that writes
// its "[]".  wiretiles.hpp's rule at t = 256: g(o) = pair_offsets[o] / 256 + o
// is strictly increasing with g(o + 1) - g(o) >= max(1, ceil(P_o / 256)), so
// workgroup w of a grid of npairs_total / 256 + n_objects owns local tile
// w - g(o) of the LAST o with g(o) <= w when that tile exists, and nothing
// otherwise.  A tile never straddles two objects, and the tiles of one object
// are consecutive workgroups: with the tiles' text lengths scanned over the
// whole grid (idle workgroups count 0), scan[g(o)] is where object o's text
// starts in that numbering and scan[g(o) + tiles_o] where it ends.
//
// DECODE.  text_offsets[o] are multiples of the 8 KiB span a decode workgroup
// parses, so span s of the buffer (bytes [8192 s, 8192 s + 8192)) lies in at
// most one slot: that of the LAST o with text_offsets[o] / 8192 <= s.  Object o
// owns max(1, ceil(text_lens[o] / 8192)) spans from its slot's first -- an
// empty text keeps one, whose workgroup reports it.  The launch covers
// texts_len / 8192 + 1 spans.
//
// Whatever the tables hold, every index stated here lies inside the arrays:
// pairs in [0, npairs_total], text bytes in [0, texts_len] or [0, out_cap),
// objects in [0, n_objects).  A table that breaks the contract misplaces or
// drops an object's data; it reads and writes nothing outside the buffers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "seglookup.hpp"

namespace amph {

constexpr size_t kXTilePairs = 256;    // kXBlock (exchange.hip asserts it)
constexpr size_t kXSlotAlign = 8192;   // AMPH_EXCHANGE_SLOT_ALIGN = kDecSpan (asserted there)
constexpr size_t kXEntryMax = 92;      // kXEntry: {"a":-<39 digits>,"b":-<39 digits>},

AMPH_SEG_HD inline uint64_t xseg_min(uint64_t a, uint64_t b) { return a < b ? a : b; }

// characters of the longest text of npairs pairs, and the dense layout's stride
AMPH_SEG_HD inline size_t xseg_max_chars(size_t npairs) { return kXEntryMax * npairs + 2; }
AMPH_SEG_HD inline size_t xseg_slot_chars(size_t npairs) {
  return (xseg_max_chars(npairs) + kXSlotAlign - 1) & ~(kXSlotAlign - 1);
}

// ---- encode ---------------------------------------------------------------------
AMPH_SEG_HD inline size_t xenc_tile_grid(uint64_t npairs_total, size_t n_objects) {
  return (size_t)(npairs_total / kXTilePairs) + n_objects;
}

// object o's pairs clamped into [0, npairs_total]: [p0, p0 + P)
AMPH_SEG_HD inline void xseg_object_pairs(const uint64_t* pair_offsets, size_t o, uint64_t npairs_total,
                                          uint64_t* p0, uint64_t* P) {
  const uint64_t a = xseg_min(pair_offsets[o], npairs_total);
  uint64_t b = xseg_min(pair_offsets[o + 1], npairs_total);
  if (b < a) b = a;
  *p0 = a;
  *P = b - a;
}

struct XEncTile {
  size_t object;     // in [0, n_objects) whatever the table holds
  bool owns;         // false: an idle workgroup (nothing read, nothing written)
  bool first;        // the object's tile 0: writes '[', ']' and out_lens[object]
  uint64_t pair0;    // first pair; pair0 + pairs <= npairs_total
  uint32_t pairs;    // 0..256 (0 only in the first tile of an object of no pairs)
  uint64_t last;     // one past the object's last pair: pair k is followed by ',' iff k + 1 < last
  size_t base_tile;  // the object's first workgroup, g(object); base_tile + tiles <= the grid
  size_t tiles;      // the object's tile count
};

// The tile of workgroup w < xenc_tile_grid(npairs_total, n_objects), n_objects >= 1.
AMPH_SEG_HD inline XEncTile xenc_tile(const uint64_t* pair_offsets, size_t n_objects, uint64_t npairs_total,
                                      size_t w) {
  // bisection over [0, n_objects) on the clamped g: pair_offsets[n_objects] is not read here
  size_t lo = 0, hi = n_objects;
  while (hi - lo > 1) {
    const size_t mid = lo + (hi - lo) / 2;
    if (xseg_min(pair_offsets[mid], npairs_total) / kXTilePairs + mid <= w) lo = mid;
    else hi = mid;
  }
  XEncTile t{lo, false, false, 0, 0, 0, 0, 0};
  uint64_t p0, P;
  xseg_object_pairs(pair_offsets, lo, npairs_total, &p0, &P);
  const uint64_t g = p0 / kXTilePairs + lo;
  t.base_tile = (size_t)g;
  t.tiles = (size_t)(P ? (P + kXTilePairs - 1) / kXTilePairs : 1);
  if (w < g || w - g >= t.tiles) return t;  // (w < g: a broken table only)
  const uint64_t local = w - g, done = kXTilePairs * local;
  t.owns = true;
  t.first = local == 0;
  t.pair0 = p0 + done;
  t.pairs = (uint32_t)xseg_min(P - done, kXTilePairs);
  t.last = p0 + P;
  return t;
}

// Where a run of `run` characters, `into` characters after the '[' of the text
// at text_offsets[o], may be stored in out[0, out_cap): the offset of its first
// character, or ~0 when any of it (or the text's closing ']' after it) would
// leave the buffer -- a broken table only; the host checks every slot first.
AMPH_SEG_HD inline uint64_t xenc_store_at(uint64_t text_offset, uint64_t into, uint64_t run, uint64_t out_cap) {
  const uint64_t none = ~(uint64_t)0;
  if (text_offset >= out_cap) return none;
  const uint64_t room = out_cap - text_offset;  // characters from the '[' on
  if (room < 2 || into > room - 2 || run > room - 2 - into) return none;
  return text_offset + 1 + into;
}

// ---- decode ---------------------------------------------------------------------
AMPH_SEG_HD inline size_t xdec_span_grid(uint64_t texts_len) { return (size_t)(texts_len / kXSlotAlign) + 1; }

struct XDecSpan {
  size_t object;    // in [0, n_objects)
  bool owns;        // false: the span lies in no text (a gap, or a slot's rest)
  uint64_t text0;   // the object's text: bytes [text0, text0 + len) of the buffer, text0 a
  uint64_t len;     //   multiple of 8192, text0 + len <= texts_len
  size_t span0;     // the object's first span, text0 / 8192; span0 + spans <= the grid
  size_t spans;     // max(1, ceil(len / 8192))
  size_t local;     // this span within the text (owns: < spans)
  uint64_t row0;    // the object's first value row, 2 * its first pair
  uint64_t nvals;   // 2 P_o: row0 + nvals <= 2 npairs_total
};

// object o's text clamped into the buffer: its slot rounded down to the span
AMPH_SEG_HD inline void xseg_object_text(const uint64_t* text_offsets, const uint64_t* text_lens, size_t o,
                                         uint64_t texts_len, uint64_t* text0, uint64_t* len) {
  const uint64_t a = xseg_min(text_offsets[o], texts_len) & ~(uint64_t)(kXSlotAlign - 1);
  *text0 = a;
  *len = xseg_min(text_lens[o], texts_len - a);
}

// Span s < xdec_span_grid(texts_len) of the buffer, n_objects >= 1.
AMPH_SEG_HD inline XDecSpan xdec_span(const uint64_t* text_offsets, const uint64_t* text_lens,
                                      const uint64_t* pair_offsets, size_t n_objects, uint64_t npairs_total,
                                      uint64_t texts_len, size_t s) {
  size_t lo = 0, hi = n_objects;
  while (hi - lo > 1) {
    const size_t mid = lo + (hi - lo) / 2;
    if (xseg_min(text_offsets[mid], texts_len) / kXSlotAlign <= s) lo = mid;
    else hi = mid;
  }
  XDecSpan d{lo, false, 0, 0, 0, 0, 0, 0, 0};
  xseg_object_text(text_offsets, text_lens, lo, texts_len, &d.text0, &d.len);
  d.span0 = (size_t)(d.text0 / kXSlotAlign);
  d.spans = (size_t)(d.len ? (d.len + kXSlotAlign - 1) / kXSlotAlign : 1);
  uint64_t p0, P;
  xseg_object_pairs(pair_offsets, lo, npairs_total, &p0, &P);
  d.row0 = 2 * p0;
  d.nvals = 2 * P;
  if (s < d.span0 || s - d.span0 >= d.spans) return d;
  d.owns = true;
  d.local = s - d.span0;
  return d;
}

}  // namespace amph
