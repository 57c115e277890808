// Geometry of the many-requests party session (amph_parties_*,
// include/amphora_party_batch.h; k_xdecs_span / k_xdecs_post in exchange.hip,
// k_open_post_seg in kernels.hip): which object's pairs an open-post workgroup
// multiplies, and where it finds a partner's values in the span form of that
// object's text.  Shared by the kernels, the session and the CPU tests, so it
// compiles for the host alone (as exchangetiles.hpp, whose decode side --
// xdec_span -- the span-form decode reuses unchanged).
//
// OPEN-POST.  pair_offsets[n_objects + 1]: 0 first, nondecreasing,
// npairs_total last; object o holds P_o pairs and is multiplied in
// ceil(P_o / 128) tiles of 128 pairs (256 values).  wiretiles.hpp's rule at
// t = 128: g(o) = pair_offsets[o] / 128 + o is strictly increasing with
// g(o + 1) - g(o) >= ceil(P_o / 128), so workgroup w of a grid of
// npairs_total / 128 + n_objects owns local tile w - g(o) of the LAST o with
// g(o) <= w when that tile exists, and nothing otherwise.  A tile never
// straddles two objects; an object of no pairs owns no tile.
//
// WINDOW.  A partner's text of object o lies in spans [span0, span0 + spans)
// of the text buffer (8 KiB each); the span pass stored the values of buffer
// span s in text order at slots [528 s, ...), and base[i] (i <= spans) is the
// scanned count in front of the object's span i.  The window of local tile t
// says where the tile's 256 values lie, with spans and value indices counted
// INSIDE THE OBJECT (the meaning of XSpans::map, kernels.hpp): x = s0, the
// object's span holding value 256 t, y = that value's rank in s0, z = o1 |
// o2 << 16 and w = o3 with o_i = base[s0 + i] - base[0] - 256 t, capped (0xFFFF
// / ~0, also past the object's last span): value 256 t + q lies in span s0 + i
// for o_i <= q < o_(i + 1) (o_0 = -y).  x = kPartyPairOrder marks an object
// whose span form does not hold: its values are in pair order elsewhere.  The
// buffer-global span number span0 + s0 + i is used only to find the slots.
//
// Whatever the tables hold, every index stated here lies inside the arrays:
// pairs in [0, npairs_total], objects in [0, n_objects), spans in [0, nb], slots
// below 528 nb when the counts in base are those of the span pass (at most 528
// per span).  A table that breaks the contract misplaces or drops an object's
// data; it reads and writes nothing outside the buffers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "exchangetiles.hpp"

namespace amph {

constexpr size_t kPartyTilePairs = 128;        // kPairBlock (kernels.hip asserts it)
constexpr size_t kPartyTileValues = 2 * kPartyTilePairs;
constexpr size_t kPartySpanSlots = 528;        // kXSpanSlots (kernels.hpp; exchange.hip asserts it)
constexpr uint32_t kPartyPairOrder = ~0u;      // window.x of an object in pair order

AMPH_SEG_HD inline size_t party_tile_grid(uint64_t npairs_total, size_t n_objects) {
  return (size_t)(npairs_total / kPartyTilePairs) + n_objects;
}

struct PartyTile {
  size_t object;   // in [0, n_objects) whatever the table holds
  bool owns;       // false: an idle workgroup (nothing read, nothing written)
  uint64_t pair0;  // first pair; pair0 + pairs <= npairs_total
  uint32_t pairs;  // 1..128 when owned
  size_t local;    // the tile within its object (owns: < ceil(P / 128))
  size_t tiles;    // the object's tile count
  size_t base_tile;  // the object's first workgroup, g(object); base_tile + tiles <= the grid
};

// The tile of workgroup w < party_tile_grid(npairs_total, n_objects), n_objects >= 1.
AMPH_SEG_HD inline PartyTile party_tile(const uint64_t* pair_offsets, size_t n_objects, uint64_t npairs_total,
                                        size_t w) {
  // bisection over [0, n_objects) on the clamped g: pair_offsets[n_objects] is read by xseg_object_pairs only
  size_t lo = 0, hi = n_objects;
  while (hi - lo > 1) {
    const size_t mid = lo + (hi - lo) / 2;
    if (xseg_min(pair_offsets[mid], npairs_total) / kPartyTilePairs + mid <= w) lo = mid;
    else hi = mid;
  }
  PartyTile t{lo, false, 0, 0, 0, 0, 0};
  uint64_t p0, P;
  xseg_object_pairs(pair_offsets, lo, npairs_total, &p0, &P);
  const uint64_t g = p0 / kPartyTilePairs + lo;
  t.base_tile = (size_t)g;
  t.tiles = (size_t)((P + kPartyTilePairs - 1) / kPartyTilePairs);
  if (w < g || w - g >= t.tiles) return t;  // (w < g: a broken table only)
  const uint64_t done = kPartyTilePairs * (w - g);
  t.owns = true;
  t.local = (size_t)(w - g);
  t.pair0 = p0 + done;
  t.pairs = (uint32_t)xseg_min(P - done, kPartyTilePairs);
  return t;
}

struct PartyWindow {
  uint32_t x, y, z, w;
};

// The window of local tile t of an object in span form.  base: the scanned
// counts at the object's first span (spans + 1 words, nondecreasing); the
// tile exists, i.e. 256 t < base[spans] - base[0].
AMPH_SEG_HD inline PartyWindow party_window(const uint64_t* base, size_t spans, size_t t) {
  const uint64_t v0 = (uint64_t)kPartyTileValues * t, b0 = base[0];
  // the LAST span i < spans with base[i] - b0 <= v0: it holds value v0 (the
  // spans without values that share its start are passed over)
  size_t lo = 0, hi = spans ? spans : 1;
  while (hi - lo > 1) {
    const size_t mid = lo + (hi - lo) / 2;
    if (base[mid] - b0 <= v0) lo = mid;
    else hi = mid;
  }
  const size_t s0 = lo;
  auto at = [&](size_t s, uint64_t cap) -> uint32_t {
    if (s > spans) return (uint32_t)cap;
    const uint64_t d = base[s] - b0 - v0;  // (>= 0 for s > s0 under the contract)
    return (uint32_t)(base[s] - b0 < v0 ? 0 : xseg_min(d, cap));
  };
  return PartyWindow{(uint32_t)s0, (uint32_t)(v0 - (base[s0] - b0)), at(s0 + 1, 0xFFFF) | (at(s0 + 2, 0xFFFF) << 16),
                     at(s0 + 3, 0xFFFFFFFFu)};
}

// The slot of value q < 256 of the tile with window w: span0 = the object's
// first span in the buffer, base as party_window's, nb = the buffer's span
// count (base[nb - span0] is the last word that exists).
AMPH_SEG_HD inline size_t party_slot(const PartyWindow& w, const uint64_t* base, size_t span0, size_t nb, size_t t,
                                     uint32_t q) {
  const size_t s0 = (size_t)w.x + span0;
  const uint32_t o1 = w.z & 0xFFFFu, o2 = w.z >> 16;
  if (q < o1) return s0 * kPartySpanSlots + w.y + q;
  if (q < o2) return (s0 + 1) * kPartySpanSlots + (q - o1);
  if (q < w.w) return (s0 + 2) * kPartySpanSlots + (q - o2);
  // a tile across more than three spans (only behind a text's short spans)
  const uint64_t v = (uint64_t)kPartyTileValues * t + q + base[0];
  size_t s = (size_t)w.x + 3;  // relative to span0
  while (span0 + s + 1 < nb && base[s + 1] <= v) ++s;
  if (span0 + s >= nb) s = nb - 1 - span0;  // (a broken window only; nb > span0)
  return (span0 + s) * kPartySpanSlots + (size_t)xseg_min(v - base[s], kPartySpanSlots - 1);
}

}  // namespace amph
