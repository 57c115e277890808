// Tile geometry of the segmented response encoder (k_odo_b64_seg, codec.hip):
// what one workgroup reads of the packed word arrays and writes of the slotted
// base64 field buffers (include/amphora_respond_batch.h).  Shared by the
// kernel, the host-side table check and the CPU tests, so it compiles for the
// host alone (as wiretiles.hpp, whose ownership rule it applies at t = 192).
//
// 192 words = 3,072 bytes = 256 twelve-byte units = 4,096 characters: tile
// `local` of object o reads words [w0 + 192 local, ...) and writes characters
// [text_offsets[o] + 4096 local, ...).  192 is a multiple of 3, so only an
// object's last tile ends in a partial unit, and its '=' count depends on the
// tile's own word count alone: W mod 3 = 1 -> "==", 2 -> "=", 0 -> none.
//
// Whatever the tables hold, a tile's words lie in [0, T] and its stored
// characters in [0, nchars): a table that breaks the contract misplaces or
// drops text, it reads nothing outside the input arrays and writes nothing
// outside the output buffers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "wiretiles.hpp"

namespace amph {

constexpr size_t kRespondTileChars = 4096;  // wire_text_chars(kWireTileWords)
// T is clamped here so that no product below can wrap (4096 T / 192 < 2^63)
constexpr uint64_t kRespondMaxWords = (uint64_t)1 << 56;

struct RespondTile {
  uint64_t in_word;   // first input word; in_word + words <= T
  uint32_t words;     // 0: no tile (nothing read, nothing written); else 1..192
  uint32_t pad;       // '=' characters that end the tile's text (0, 1 or 2)
  uint64_t out_char;  // first output character; out_char + store <= nchars
  uint32_t chars;     // characters of the tile's text: wire_text_chars(words)
  uint32_t store;     // of those, the leading ones that are stored (clipped to nchars)
  bool first;         // tile 0 of its object: the owner of a rejected object's "!!!!"
  // the workgroup-staged path: 256 whole units, nothing clipped, aligned stores
  AMPH_SEG_HD bool whole() const {
    return words == kWireTileWords && store == kRespondTileChars && (out_char & 15) == 0;
  }
};

// object o's word range clamped into [0, T]: [w0, w0 + W)
AMPH_SEG_HD inline void respond_object_words(const uint64_t* word_offsets, size_t o, uint64_t T, uint64_t* w0,
                                             uint64_t* W) {
  if (T > kRespondMaxWords) T = kRespondMaxWords;
  const uint64_t a = word_offsets[o] < T ? word_offsets[o] : T;
  uint64_t b = word_offsets[o + 1] < T ? word_offsets[o + 1] : T;
  if (b < a) b = a;
  *w0 = a;
  *W = b - a;
}

// Tile `local` of object o (what wire_tile_find returned for a workgroup).
AMPH_SEG_HD inline RespondTile respond_tile(const uint64_t* word_offsets, const uint64_t* text_offsets, size_t o,
                                            size_t local, uint64_t T, uint64_t nchars) {
  RespondTile t{0, 0, 0, 0, 0, 0, false};
  uint64_t w0, W;
  respond_object_words(word_offsets, o, T, &w0, &W);
  if (!wire_tile_real(local, W)) return t;  // (compared in tiles: local may be near 2^64)
  const uint64_t done = (uint64_t)kWireTileWords * local;  // < W <= 2^56
  t.in_word = w0 + done;
  t.words = (uint32_t)(W - done < kWireTileWords ? W - done : kWireTileWords);
  t.pad = (3 - t.words % 3) % 3;
  t.chars = (uint32_t)wire_text_chars(t.words);
  t.first = local == 0;
  const uint64_t into = (uint64_t)kRespondTileChars * local;  // < 2^63
  const uint64_t at = text_offsets[o] + into;
  t.out_char = at;
  if (at < into || at >= nchars) t.store = 0;  // the sum wrapped, or the tile starts past the buffers
  else t.store = (uint32_t)(nchars - at < t.chars ? nchars - at : t.chars);
  if (!t.store) t.out_char = 0;
  return t;
}

}  // namespace amph
