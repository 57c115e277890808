// Stand-alone host driver of amphora_amd/csrc/respondtiles.hpp
// (tests/test_respond_batch_cpu.py): the tile geometry of k_odo_b64_seg, which
// writes many objects' base64 field texts into slotted buffers in one launch.
// No library is linked.
//
//   respondtiles_test                  every check below, "respondtiles ok" on success
//   respondtiles_test tables T NCHARS K w0..wK t0..t(K-1)
//                                      one table, contract or not: every workgroup's
//                                      tile must stay inside [0, T] and [0, NCHARS);
//                                      prints "inside" or the breach
//
// Honest tables, against a linear enumeration: every workgroup w of the grid
// T / 192 + n_objects is looked up (wire_tile_find) and its tile stated
// (respond_tile); every character of every text is stored by exactly one
// tile, no character of a gap or behind the last text by any; each tile reads
// exactly the words whose bytes its characters encode; the '=' count is the
// text's; a tile takes the staged path iff it is 192 whole words.
// Hostile tables (decreasing, offsets near 2^64, texts past nchars, unaligned
// slots): no tile reads outside [0, T] or stores outside [0, nchars).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "respondtiles.hpp"

namespace {
long g_tables = 0, g_hostile = 0;

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return rng_state * 0x2545F4914F6CDD1Dull;
}

// words[o] per object, gap[o] = unused characters (a multiple of 16) after
// object o's slot, tail = characters after the last slot
bool check(const std::vector<uint64_t>& words, const std::vector<uint64_t>& gap, uint64_t tail, const char* what) {
  const size_t K = words.size();
  std::vector<uint64_t> woff(K + 1, 0), toff(K, 0);
  uint64_t at = 0;
  for (size_t o = 0; o < K; ++o) {
    woff[o + 1] = woff[o] + words[o];
    toff[o] = at;
    at += amph::wire_slot_chars(words[o]) + gap[o];
  }
  const uint64_t T = woff[K], nchars = at + tail;
  std::vector<uint8_t> owners(nchars, 0), wanted(nchars, 0);
  for (size_t o = 0; o < K; ++o)
    for (uint64_t c = 0; c < amph::wire_text_chars(words[o]); ++c) wanted[toff[o] + c] = 1;
  const size_t grid = amph::wire_tile_grid(T, K);
  for (size_t w = 0; w < grid; ++w) {
    const amph::WireTile wt = amph::wire_tile_find(woff.data(), K, w);
    if (wt.object >= K) return std::printf("%s: w %zu gives object %zu of %zu\n", what, w, wt.object, K), false;
    const amph::RespondTile t = amph::respond_tile(woff.data(), toff.data(), wt.object, wt.local, T, nchars);
    const uint64_t W = words[wt.object];
    const bool real = amph::wire_tile_real(wt.local, W);
    if (real != (t.words != 0))
      return std::printf("%s: w %zu real %d, tile of %u words\n", what, w, (int)real, t.words), false;
    if (!real) {
      if (t.store || t.chars) return std::printf("%s: w %zu has no tile but stores\n", what, w), false;
      continue;
    }
    const uint64_t done = 192 * (uint64_t)wt.local, left = W - done;
    const bool last = left <= 192;
    const uint64_t want_words = last ? left : 192;
    const uint64_t want_chars = last ? amph::wire_text_chars(W) - 4096 * (uint64_t)wt.local : 4096;
    const uint32_t want_pad = last ? (uint32_t)((3 - (16 * W) % 3) % 3) : 0;
    if (t.in_word != woff[wt.object] + done || t.words != want_words || t.chars != want_chars ||
        t.store != want_chars || t.pad != want_pad || t.out_char != toff[wt.object] + 4096 * (uint64_t)wt.local ||
        t.first != (wt.local == 0) || t.whole() != (want_words == 192)) {
      std::printf("%s: w %zu tile (%zu, %zu): words %u@%llu chars %u store %u pad %u at %llu whole %d\n", what, w,
                  wt.object, wt.local, t.words, (unsigned long long)t.in_word, t.chars, t.store, t.pad,
                  (unsigned long long)t.out_char, (int)t.whole());
      return false;
    }
    // the characters encode exactly the tile's bytes: 4 per 3, the last group padded
    if (t.chars != 4 * ((16 * (uint64_t)t.words + 2) / 3) ||
        3 * (uint64_t)(t.chars / 4) - t.pad != 16 * (uint64_t)t.words)
      return std::printf("%s: w %zu: %u characters, %u pads for %u words\n", what, w, t.chars, t.pad, t.words), false;
    for (uint64_t c = 0; c < t.store; ++c)
      if (++owners[t.out_char + c] > 1)
        return std::printf("%s: character %llu has two owners\n", what, (unsigned long long)(t.out_char + c)), false;
  }
  for (uint64_t c = 0; c < nchars; ++c)
    if (owners[c] != wanted[c])
      return std::printf("%s: character %llu: %d owners, %d wanted\n", what, (unsigned long long)c, owners[c],
                         wanted[c]),
             false;
  ++g_tables;
  return true;
}

// any table at all: every workgroup of a generous grid stays inside
bool inside(const std::vector<uint64_t>& woff, const std::vector<uint64_t>& toff, uint64_t T, uint64_t nchars,
            bool print) {
  const size_t K = toff.size();
  const uint64_t Tc = T < amph::kRespondMaxWords ? T : amph::kRespondMaxWords;
  size_t grid = amph::wire_tile_grid(Tc, K) + 3;
  if (grid > 200000) grid = 200000;
  for (size_t w = 0; w < grid; ++w) {
    const amph::WireTile wt = amph::wire_tile_find(woff.data(), K, w);
    if (wt.object >= K) return print && std::printf("w %zu: object %zu of %zu\n", w, wt.object, K), false;
    // the kernel's own locals, and the extremes a broken lookup could produce
    for (size_t local : {wt.local, (size_t)0, (size_t)1, ~(size_t)0, (size_t)1 << 63, (size_t)(Tc / 192)}) {
      const amph::RespondTile t = amph::respond_tile(woff.data(), toff.data(), wt.object, local, T, nchars);
      const bool ok = t.words <= 192 && t.in_word <= T && t.words <= T - t.in_word && t.store <= t.chars &&
                      t.chars <= 4096 && t.out_char <= nchars && t.store <= nchars - t.out_char &&
                      (t.words || !t.store) && t.pad <= 2;
      if (!ok) {
        if (print)
          std::printf("w %zu local %zu: words [%llu, +%u) of %llu, characters [%llu, +%u) of %llu\n", w, local,
                      (unsigned long long)t.in_word, t.words, (unsigned long long)T, (unsigned long long)t.out_char,
                      t.store, (unsigned long long)nchars);
        return false;
      }
      if (t.whole() && ((t.out_char & 15) || t.store != 4096 || t.words != 192)) return false;
    }
  }
  ++g_hostile;
  return true;
}

const uint64_t kCounts[] = {0, 1, 2, 3, 191, 192, 193, 0, 385, 576, 0};
constexpr size_t kN = sizeof(kCounts) / sizeof(kCounts[0]);

bool honest() {
  const std::vector<uint64_t> suite(kCounts, kCounts + kN);
  for (uint64_t g : {(uint64_t)0, (uint64_t)16, (uint64_t)48})
    for (uint64_t tail : {(uint64_t)0, (uint64_t)16, (uint64_t)4096})
      if (!check(suite, std::vector<uint64_t>(kN, g), tail, "suite sizes")) return false;
  for (size_t K : {(size_t)1, (size_t)2, (size_t)3, (size_t)64, (size_t)300})
    for (size_t shift = 0; shift < kN; ++shift) {
      std::vector<uint64_t> w(K), g(K);
      for (size_t o = 0; o < K; ++o) {
        w[o] = kCounts[(o + shift) % kN];
        g[o] = 16 * ((o + shift) % 4);
      }
      if (!check(w, g, 16 * shift, "cycle")) return false;
      if (!check(std::vector<uint64_t>(K, kCounts[shift]), std::vector<uint64_t>(K, 0), 0, "uniform")) return false;
    }
  for (int it = 0; it < 3000; ++it) {
    const size_t K = 1 + rnd() % 24;
    std::vector<uint64_t> w(K), g(K);
    for (size_t o = 0; o < K; ++o) {
      const uint64_t r = rnd() % 8;
      w[o] = r < 2 ? 0 : r < 4 ? kCounts[rnd() % kN] : r < 7 ? rnd() % 600 : 1000 + rnd() % 3000;
      g[o] = 16 * (rnd() % 5);
    }
    if (!check(w, g, 16 * (rnd() % 3), "random")) return false;
  }
  return true;
}

uint64_t hostile_value(uint64_t T, uint64_t nchars) {
  switch (rnd() % 8) {
    case 0: return ~(uint64_t)0 - rnd() % 5000;
    case 1: return ((uint64_t)1 << 63) + rnd() % 5000 - 2500;
    case 2: return T + rnd() % 400;
    case 3: return nchars + rnd() % 5000;
    case 4: return nchars - (nchars ? rnd() % (nchars < 5000 ? nchars : 5000) : 0);
    case 5: return rnd();
    default: return rnd() % (T + 200);
  }
}

bool hostile() {
  for (int it = 0; it < 10000; ++it) {
    const size_t K = 1 + rnd() % 12;
    const uint64_t T = it % 50 == 0 ? ~(uint64_t)0 >> (rnd() % 8) : rnd() % 3000;
    const uint64_t nchars = it % 70 == 0 ? ~(uint64_t)0 - rnd() % 4096 : rnd() % 70000;
    std::vector<uint64_t> woff(K + 1), toff(K);
    for (auto& x : woff) x = hostile_value(T, nchars);
    for (auto& x : toff) x = hostile_value(T, nchars);
    if (it % 3 == 0) {  // an honest word table under hostile slots, and the other way round
      woff[0] = 0;
      for (size_t o = 0; o < K; ++o) woff[o + 1] = woff[o] + rnd() % 400;
    }
    if (it % 3 == 1)
      for (size_t o = 0; o < K; ++o) toff[o] = 16 * (rnd() % 4000);
    if (!inside(woff, toff, T, nchars, true)) {
      std::printf("hostile table %d breaks out\n", it);
      return false;
    }
  }
  return true;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc > 4 && !std::strcmp(argv[1], "tables")) {
    const uint64_t T = std::strtoull(argv[2], nullptr, 10), nchars = std::strtoull(argv[3], nullptr, 10);
    const size_t K = std::strtoull(argv[4], nullptr, 10);
    if (K == 0 || (size_t)argc != 5 + 2 * K + 1) return std::printf("usage: tables T NCHARS K w0..wK t0..t(K-1)\n"), 2;
    std::vector<uint64_t> woff(K + 1), toff(K);
    for (size_t i = 0; i <= K; ++i) woff[i] = std::strtoull(argv[5 + i], nullptr, 10);
    for (size_t i = 0; i < K; ++i) toff[i] = std::strtoull(argv[6 + K + i], nullptr, 10);
    if (!inside(woff, toff, T, nchars, true)) return 1;
    std::printf("inside\n");
    return 0;
  }
  if (!honest() || !hostile()) return 1;
  std::printf("respondtiles ok (%ld tables, %ld hostile)\n", g_tables, g_hostile);
  return 0;
}
