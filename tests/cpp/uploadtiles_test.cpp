// Stand-alone host driver of amphora_amd/csrc/wiretiles.hpp at the tile sizes
// of the upload batch kernels (tests/test_upload_batch_cpu.py): k_conv_json_seg
// looks its tile up at t = 128, k_mask_json_seg at t = 192, and both give an
// object of no words -- which has no tile but still a text, "[]" -- to
// workgroup g(o) = offsets[o] / t + o.  No library is linked.
//
//   uploadtiles_test            every check below, "uploadtiles ok" on success
//   uploadtiles_test slot W..   W, masked_input_data_chars(W), upload_slot_chars(W)
//
// For every table and both t, against a linear enumeration: each workgroup w
// of the grid T / t + n_objects is looked up; every real tile (o, local) is
// owned exactly once, every other w finds no tile, and every empty object's
// g(o) lies in the grid, resolves to (o, 0) and is no real tile's workgroup --
// so exactly one workgroup handles its "[]".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <utility>
#include <vector>

#include "wiretiles.hpp"

namespace {
long g_tables = 0;

uint64_t rng_state = 0xD1B54A32D192ED03ull;
uint64_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return rng_state * 0x2545F4914F6CDD1Dull;
}

bool check(const std::vector<uint64_t>& words, size_t t, const char* what) {
  const size_t K = words.size();
  std::vector<uint64_t> off(K + 1, 0);
  for (size_t o = 0; o < K; ++o) off[o + 1] = off[o] + words[o];
  // the lookup never reads entry K: it lives outside this exact-size array
  std::vector<uint64_t> tab(off.begin(), off.begin() + K);
  const size_t grid = amph::wire_tile_grid(off[K], K, t);
  // the linear enumeration: tiles in object order, each at g(o) + local
  std::map<size_t, std::pair<size_t, size_t>> want;  // workgroup -> (object, local)
  std::set<size_t> empties;                          // workgroups g(o) of the empty objects
  for (size_t o = 0; o < K; ++o) {
    const size_t g = (size_t)(off[o] / t) + o;
    if (words[o] == 0) {
      if (g >= grid || !empties.insert(g).second) {
        std::printf("%s t=%zu: empty object %zu at workgroup %zu of %zu\n", what, t, o, g, grid);
        return false;
      }
    }
    for (size_t l = 0; l * t < words[o]; ++l)
      if (g + l >= grid || !want.emplace(g + l, std::make_pair(o, l)).second) {
        std::printf("%s t=%zu: tile (%zu, %zu) at workgroup %zu collides or leaves the grid %zu\n", what, t, o, l,
                    g + l, grid);
        return false;
      }
  }
  for (size_t g : empties)
    if (want.count(g)) {
      std::printf("%s t=%zu: an empty object's workgroup %zu is a real tile's\n", what, t, g);
      return false;
    }
  size_t empty_seen = 0;
  for (size_t w = 0; w < grid; ++w) {
    const amph::WireTile wt = amph::wire_tile_find(tab.data(), K, w, t);
    if (wt.object >= K) {
      std::printf("%s t=%zu: w %zu gives object %zu of %zu\n", what, t, w, wt.object, K);
      return false;
    }
    const bool real = amph::wire_tile_real(wt.local, words[wt.object], t);
    const auto it = want.find(w);
    if (real != (it != want.end()) ||
        (real && (it->second.first != wt.object || it->second.second != wt.local))) {
      std::printf("%s t=%zu: w %zu found (%zu, %zu) real %d, enumeration differs\n", what, t, w, wt.object, wt.local,
                  (int)real);
      return false;
    }
    // the kernels' rule for "[]": an object of no words whose local tile is 0
    if (words[wt.object] == 0 && wt.local == 0) {
      if (!empties.count(w)) {
        std::printf("%s t=%zu: w %zu claims empty object %zu, not its g(o)\n", what, t, w, wt.object);
        return false;
      }
      ++empty_seen;
    }
  }
  if (empty_seen != empties.size()) {
    std::printf("%s t=%zu: %zu empty objects handled, %zu exist\n", what, t, empty_seen, empties.size());
    return false;
  }
  ++g_tables;
  return true;
}

bool check_both(const std::vector<uint64_t>& w, const char* what) {
  return check(w, amph::kConvTileWords, what) && check(w, amph::kWireTileWords, what);
}

const uint64_t kCounts[] = {0, 1, 2, 127, 128, 129, 191, 192, 193, 257, 385};
constexpr size_t kN = sizeof(kCounts) / sizeof(kCounts[0]);

bool shapes() {
  // the suites' own tables
  if (!check_both({0, 1, 2, 127, 128, 129, 0, 257, 1}, "convert sizes")) return false;
  if (!check_both({0, 1, 191, 192, 193, 0, 385}, "mask sizes")) return false;
  for (size_t K : {(size_t)1, (size_t)2, (size_t)3, (size_t)64, (size_t)500}) {
    for (size_t shift = 0; shift < kN; ++shift) {
      std::vector<uint64_t> w(K);
      for (size_t o = 0; o < K; ++o) w[o] = kCounts[(o + shift) % kN];
      if (!check_both(w, "cycle")) return false;
    }
    for (uint64_t c : kCounts) {
      if (!check_both(std::vector<uint64_t>(K, c), "uniform")) return false;
      for (int where = 0; where < 4; ++where) {  // empty objects first, in the middle, last, in runs
        std::vector<uint64_t> v(K, c ? c : 129);
        for (size_t o = 0; o < K; ++o) {
          const bool hole = where == 0 ? o < (K + 2) / 3
                          : where == 1 ? (o >= K / 3 && o < K - K / 3 && K > 2)
                          : where == 2 ? o >= K - (K + 2) / 3
                                       : (o / 3) % 2 == 0;
          if (hole) v[o] = 0;
        }
        if (!check_both(v, "holes")) return false;
      }
    }
  }
  return true;
}

bool random_tables() {
  for (int it = 0; it < 12000; ++it) {
    const size_t K = 1 + rnd() % 40;
    std::vector<uint64_t> w(K);
    for (size_t o = 0; o < K; ++o) {
      const uint64_t r = rnd() % 8;
      w[o] = r < 3 ? 0 : r < 5 ? kCounts[rnd() % kN] : r < 7 ? rnd() % 600 : 1000 + rnd() % 5000;
    }
    if (!check_both(w, "random")) return false;
  }
  return true;
}

bool slots() {
  for (uint64_t w = 0; w < 2000; ++w) {
    const size_t nc = amph::masked_input_data_chars(w), sl = amph::upload_slot_chars(w);
    if (nc != (w ? 37 * w + 1 : 2) || sl % 16 || sl < nc || sl >= nc + 16) {
      std::printf("upload slot chars of %llu words: %zu / %zu\n", (unsigned long long)w, nc, sl);
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
      std::printf("%zu %zu %zu\n", w, amph::masked_input_data_chars(w), amph::upload_slot_chars(w));
    }
    return 0;
  }
  if (!shapes() || !random_tables() || !slots()) return 1;
  std::printf("uploadtiles ok (%ld tables)\n", g_tables);
  return 0;
}
