// Stand-alone host driver of amphora_amd/csrc/wiretiles.hpp
// (tests/test_wire_batch_cpu.py): the tile ownership rule of the segmented
// wire-text kernels against a linear enumeration.  No library is linked.
//
//   wiretiles_test            every check below, "wiretiles ok" on success
//   wiretiles_test slot W..   amph::wire_slot_chars / wire_text_chars of each W
//
// For every table: each workgroup w of the grid T / t + n_objects is looked up;
// every real tile (o, local) must be owned exactly once and every other w must
// find no tile.  Tables: the required word counts in every position with empty
// objects at the start, in the middle, at the end and in runs, 1 / 2 / 3 / 64 /
// 1,000 objects, 20,000 random tables, and tables that break the contract
// (which must still give an object in range).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "wiretiles.hpp"

namespace {
constexpr size_t t = amph::kWireTileWords;
long g_tables = 0;

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return rng_state * 0x2545F4914F6CDD1Dull;
}

bool check(const std::vector<uint64_t>& words, const char* what) {
  const size_t K = words.size();
  std::vector<uint64_t> off(K + 1, 0);
  for (size_t o = 0; o < K; ++o) off[o + 1] = off[o] + words[o];
  // the table the lookup sees ends at off[K - 1]: entry K must never be read,
  // so it lives outside this exact-size array (ASan catches a read of it)
  std::vector<uint64_t> tab(off.begin(), off.begin() + K);
  std::map<std::pair<size_t, size_t>, int> owned;
  const size_t grid = amph::wire_tile_grid(off[K], K);
  for (size_t w = 0; w < grid; ++w) {
    const amph::WireTile wt = amph::wire_tile_find(tab.data(), K, w);
    if (wt.object >= K) {
      std::printf("%s: w %zu gives object %zu of %zu\n", what, w, wt.object, K);
      return false;
    }
    if (amph::wire_tile_real(wt.local, words[wt.object])) ++owned[{wt.object, wt.local}];
  }
  size_t real = 0;
  for (size_t o = 0; o < K; ++o)
    for (size_t l = 0; l * t < words[o]; ++l, ++real) {
      const auto it = owned.find({o, l});
      if (it == owned.end() || it->second != 1) {
        std::printf("%s: tile (%zu, %zu) owned %d times\n", what, o, l, it == owned.end() ? 0 : it->second);
        return false;
      }
    }
  if (owned.size() != real) {
    std::printf("%s: %zu tiles owned, %zu exist\n", what, owned.size(), real);
    return false;
  }
  ++g_tables;
  return true;
}

const uint64_t kCounts[] = {0, 1, 191, 192, 193, 383, 384, 385};

bool shapes() {
  for (size_t K : {(size_t)1, (size_t)2, (size_t)3, (size_t)64, (size_t)1000}) {
    // every count in every position, the others cycling through the list
    for (size_t shift = 0; shift < 8; ++shift) {
      std::vector<uint64_t> w(K);
      for (size_t o = 0; o < K; ++o) w[o] = kCounts[(o + shift) % 8];
      if (!check(w, "cycle")) return false;
    }
    for (uint64_t c : kCounts) {
      std::vector<uint64_t> w(K, c);  // uniform
      if (!check(w, "uniform")) return false;
      // empty objects at the start, in the middle, at the end and in runs
      for (int where = 0; where < 4; ++where) {
        std::vector<uint64_t> v(K, c ? c : 193);
        for (size_t o = 0; o < K; ++o) {
          const bool hole = where == 0 ? o < (K + 2) / 3
                          : where == 1 ? (o >= K / 3 && o < K - K / 3 && K > 2)
                          : where == 2 ? o >= K - (K + 2) / 3
                                       : (o / 3) % 2 == 0;
          if (hole) v[o] = 0;
        }
        if (!check(v, "holes")) return false;
      }
    }
    if (!check(std::vector<uint64_t>(K, 0), "all empty")) return false;
  }
  return true;
}

bool random_tables() {
  for (int it = 0; it < 20000; ++it) {
    const size_t K = 1 + rnd() % 40;
    std::vector<uint64_t> w(K);
    for (size_t o = 0; o < K; ++o) {
      const uint64_t r = rnd() % 8;
      w[o] = r < 2 ? 0 : r < 5 ? kCounts[rnd() % 8] : r < 7 ? rnd() % 600 : 1000 + rnd() % 9000;
    }
    if (!check(w, "random")) return false;
  }
  return true;
}

// tables that break the contract: the object stays in [0, n_objects), and a
// tile that comes out real lies inside that object's own claimed words
bool broken_tables() {
  for (int it = 0; it < 2000; ++it) {
    const size_t K = 1 + rnd() % 20;
    std::vector<uint64_t> tab(K);
    for (size_t o = 0; o < K; ++o) tab[o] = it % 4 == 0 ? rnd() : rnd() % 5000;  // not sorted, tab[0] != 0
    for (uint64_t w = 0; w < 200; ++w) {
      const amph::WireTile wt = amph::wire_tile_find(tab.data(), K, it % 2 ? w : rnd());
      if (wt.object >= K) {
        std::printf("broken table: object %zu of %zu\n", wt.object, K);
        return false;
      }
      // wire_tile_real compares tiles, so a wrapped local is never real for any plausible count
      if (wt.local > (1ull << 60) && amph::wire_tile_real(wt.local, 1ull << 40)) {
        std::printf("broken table: a wrapped local tile counted as real\n");
        return false;
      }
    }
  }
  return true;
}

bool slots() {
  for (uint64_t w = 0; w < 2000; ++w) {
    const size_t nc = amph::wire_text_chars(w), sl = amph::wire_slot_chars(w);
    const size_t want = 4 * ((16 * w + 2) / 3);
    if (nc != want || sl % 16 || sl < nc || sl >= nc + 16) {
      std::printf("slot chars of %llu words: %zu / %zu\n", (unsigned long long)w, nc, sl);
      return false;
    }
  }
  return true;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && !std::strcmp(argv[1], "slot")) {
    for (int i = 2; i < argc; ++i) {
      const size_t w = std::strtoull(argv[i], nullptr, 10);
      std::printf("%zu %zu %zu\n", w, amph::wire_text_chars(w), amph::wire_slot_chars(w));
    }
    return 0;
  }
  if (!shapes() || !random_tables() || !broken_tables() || !slots()) return 1;
  std::printf("wiretiles ok (%ld tables)\n", g_tables);
  return 0;
}
