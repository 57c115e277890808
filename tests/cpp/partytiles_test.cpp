// Stand-alone host driver of amphora_amd/csrc/partytiles.hpp
// (tests/test_party_batch_cpu.py): which object's pairs an open-post workgroup
// of the party batch session multiplies, and where a tile finds a partner's
// values in the span form.  No library is linked.
//
//   partytiles_test        every check below, "partytiles ok" on success
//
// Honest tables, against a linear enumeration.  Tiles: every workgroup w of the
// grid npairs / 128 + n_objects is looked up (party_tile); every pair has
// exactly one owner, in its own object; no tile holds pairs of two objects; an
// object's tiles are consecutive workgroups from base_tile; an object of no
// pairs owns no tile.  Windows: an object's spans get random counts (none,
// few, 528), behind a prefix that carries other objects' counts and fail
// bits; every value of every tile must be found at the slot a walk over the
// spans gives (party_window + party_slot), tiles across more than three
// spans included.
// Hostile tables (decreasing, past the end, 2^64 - 1): no index outside
// [0, npairs], [0, n_objects) or the grid; hostile span ranges over honest
// counts: every slot below 528 nb and nothing read outside base's nb + 1
// words (the arrays are allocated exactly, for the sanitizer).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "partytiles.hpp"

namespace {
long g_tables = 0, g_windows = 0, g_hostile = 0;

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return rng_state * 0x2545F4914F6CDD1Dull;
}

#define FAIL(...) return std::printf(__VA_ARGS__), std::printf("\n"), false

bool check_tiles(const std::vector<uint64_t>& pairs, const char* what) {
  const size_t K = pairs.size();
  std::vector<uint64_t> poff(K + 1, 0);
  for (size_t o = 0; o < K; ++o) poff[o + 1] = poff[o] + pairs[o];
  const uint64_t T = poff[K];
  std::vector<uint8_t> owners(T, 0);
  std::vector<size_t> tiles(K, 0);
  const size_t grid = amph::party_tile_grid(T, K);
  for (size_t w = 0; w < grid; ++w) {
    const amph::PartyTile t = amph::party_tile(poff.data(), K, T, w);
    if (t.object >= K) FAIL("%s: w %zu gives object %zu of %zu", what, w, t.object, K);
    if (t.base_tile + t.tiles > grid) FAIL("%s: w %zu: tiles [%zu, +%zu) leave the grid %zu", what, w, t.base_tile, t.tiles, grid);
    if (!t.owns) continue;
    const size_t o = t.object;
    if (t.base_tile != poff[o] / 128 + o || t.tiles != (pairs[o] + 127) / 128 || t.local != w - t.base_tile ||
        t.local >= t.tiles)
      FAIL("%s: w %zu: object %zu base %zu tiles %zu local %zu", what, w, o, t.base_tile, t.tiles, t.local);
    const uint64_t done = 128 * (uint64_t)t.local;
    if (t.pair0 != poff[o] + done || t.pairs != (pairs[o] - done < 128 ? pairs[o] - done : 128) || t.pairs == 0)
      FAIL("%s: w %zu: pairs [%llu, +%u)", what, w, (unsigned long long)t.pair0, t.pairs);
    ++tiles[o];
    for (uint64_t k = 0; k < t.pairs; ++k) {
      if (t.pair0 + k < poff[o] || t.pair0 + k >= poff[o + 1]) FAIL("%s: w %zu straddles two objects", what, w);
      if (++owners[t.pair0 + k] > 1) FAIL("%s: pair %llu has two owners", what, (unsigned long long)(t.pair0 + k));
    }
  }
  for (uint64_t k = 0; k < T; ++k)
    if (owners[k] != 1) FAIL("%s: pair %llu has no owner", what, (unsigned long long)k);
  for (size_t o = 0; o < K; ++o)
    if (tiles[o] != (pairs[o] + 127) / 128) FAIL("%s: object %zu: %zu tiles", what, o, tiles[o]);
  ++g_tables;
  return true;
}

// an object of `counts.size()` spans at span0 of a buffer of nb spans
bool check_windows(const std::vector<uint32_t>& counts, size_t span0, size_t tail, uint64_t prefix, const char* what) {
  const size_t spans = counts.size(), nb = span0 + spans + tail;
  std::vector<uint64_t> bscan(nb + 1);
  uint64_t run = prefix;
  for (size_t s = 0; s <= nb; ++s) {
    bscan[s] = run;
    if (s < span0) run += rnd() % 529 + ((rnd() % 5 == 0) ? ((uint64_t)1 << 40) : 0);
    else if (s < span0 + spans) run += counts[s - span0];
    else run += rnd() % 529;
  }
  const uint64_t* base = bscan.data() + span0;
  const uint64_t total = base[spans] - base[0];
  // the walk: value v lies in span i at rank r
  std::vector<size_t> want(total);
  {
    uint64_t v = 0;
    for (size_t i = 0; i < spans; ++i)
      for (uint32_t r = 0; r < counts[i]; ++r) want[v++] = (span0 + i) * amph::kPartySpanSlots + r;
  }
  const size_t tiles = (size_t)((total + 255) / 256);
  for (size_t t = 0; t < tiles; ++t) {
    const amph::PartyWindow w = amph::party_window(base, spans, t);
    if (w.x >= spans || w.x == amph::kPartyPairOrder) FAIL("%s: tile %zu starts in span %u of %zu", what, t, w.x, spans);
    for (uint32_t q = 0; q < 256 && 256 * (uint64_t)t + q < total; ++q) {
      const size_t got = amph::party_slot(w, base, span0, nb, t, q);
      if (got != want[256 * t + q])
        FAIL("%s: tile %zu value %u: slot %zu, wanted %zu (window %u %u %u|%u %u)", what, t, q, got, want[256 * t + q],
             w.x, w.y, w.z & 0xFFFF, w.z >> 16, w.w);
    }
  }
  ++g_windows;
  return true;
}

const uint64_t kPairs[] = {0, 1, 127, 128, 129, 0, 0, 255, 256, 257, 700, 0};
constexpr size_t kNP = sizeof(kPairs) / sizeof(kPairs[0]);

bool honest() {
  if (!check_tiles(std::vector<uint64_t>(kPairs, kPairs + kNP), "suite sizes")) return false;
  for (size_t K : {(size_t)1, (size_t)2, (size_t)3, (size_t)64, (size_t)300})
    for (size_t shift = 0; shift < kNP; ++shift) {
      std::vector<uint64_t> p(K);
      for (size_t o = 0; o < K; ++o) p[o] = kPairs[(o + shift) % kNP];
      if (!check_tiles(p, "cycle") || !check_tiles(std::vector<uint64_t>(K, kPairs[shift]), "uniform")) return false;
    }
  for (int it = 0; it < 4000; ++it) {
    const size_t K = 1 + rnd() % 24;
    std::vector<uint64_t> p(K);
    uint64_t empty_run = 0;
    for (size_t o = 0; o < K; ++o) {
      const uint64_t r = rnd() % 8;
      if (empty_run) {  // runs of empty objects
        p[o] = 0;
        --empty_run;
        continue;
      }
      if (r == 0) empty_run = rnd() % 5;
      p[o] = r < 2 ? 0 : r < 4 ? kPairs[rnd() % kNP] : r < 7 ? rnd() % 800 : 1000 + rnd() % 3000;
    }
    if (!check_tiles(p, "random")) return false;
  }
  for (int it = 0; it < 3000; ++it) {
    const size_t spans = 1 + rnd() % 12;
    std::vector<uint32_t> c(spans);
    const int kind = (int)(rnd() % 4);
    for (auto& x : c) {
      const uint64_t r = rnd() % 8;
      if (kind == 0) x = 167 + (uint32_t)(rnd() % 362);                       // full spans of a real text
      else if (kind == 1) x = r < 3 ? 0 : (uint32_t)(rnd() % 40);            // short spans: tiles across many
      else x = r == 0 ? 0 : r == 1 ? 528 : r == 2 ? 1 : (uint32_t)(rnd() % 529);
    }
    const uint64_t prefix = rnd() % 3 ? rnd() % 100000 : (rnd() % 7 << 40) + rnd() % 100000;
    if (!check_windows(c, rnd() % 5, rnd() % 3, prefix, "random")) return false;
  }
  return true;
}

uint64_t hostile_value(uint64_t a) {
  switch (rnd() % 7) {
    case 0: return ~(uint64_t)0 - rnd() % 5000;
    case 1: return ((uint64_t)1 << 63) + rnd() % 5000 - 2500;
    case 2: return a + rnd() % 400;
    case 3: return a - (a ? rnd() % (a < 400 ? a : 400) : 0);
    case 4: return rnd();
    default: return rnd() % (a + 200);
  }
}

bool hostile() {
  for (int it = 0; it < 10000; ++it) {
    const size_t K = 1 + rnd() % 12;
    const uint64_t npairs = it % 50 == 0 ? ((uint64_t)1 << 40) + rnd() % 1000 : rnd() % 3000;
    std::vector<uint64_t> poff(K + 1);
    for (auto& x : poff) x = hostile_value(npairs);
    if (it % 4 == 0) std::sort(poff.rbegin(), poff.rend());  // decreasing
    size_t grid = amph::party_tile_grid(npairs, K);
    const size_t full = grid;
    if (grid > 50000) grid = 50000;
    for (size_t w = 0; w < grid; ++w) {
      const amph::PartyTile t = amph::party_tile(poff.data(), K, npairs, w);
      const bool ok = t.object < K && t.pairs <= 128 && t.pair0 <= npairs && t.pairs <= npairs - t.pair0 &&
                      (t.owns ? t.pairs >= 1 && t.base_tile + t.local == w && t.local < t.tiles : t.pairs == 0) &&
                      t.base_tile + t.tiles <= full;
      if (!ok) FAIL("hostile %d, w %zu: object %zu pairs [%llu, +%u) of %llu, tiles [%zu, +%zu)", it, w, t.object,
                    (unsigned long long)t.pair0, t.pairs, (unsigned long long)npairs, t.base_tile, t.tiles);
    }
    // honest counts (the span pass's: at most 528 per span), any span range inside the grid
    const size_t nb = 1 + rnd() % 40;
    std::vector<uint64_t> bscan(nb + 1);
    uint64_t run = rnd() % 3 ? 0 : rnd() << 20;
    for (size_t s = 0; s <= nb; ++s) {
      bscan[s] = run;
      run += rnd() % 529;
    }
    const size_t span0 = rnd() % nb, spans = rnd() % (nb - span0 + 1);
    const uint64_t* base = bscan.data() + span0;
    const uint64_t total = base[spans] - base[0];
    for (size_t t = 0; 256 * t < total; ++t) {
      const amph::PartyWindow w = amph::party_window(base, spans, t);
      for (uint32_t q = 0; q < 256 && 256 * (uint64_t)t + q < total; ++q)
        if (amph::party_slot(w, base, span0, nb, t, q) >= amph::kPartySpanSlots * nb)
          FAIL("hostile %d: tile %zu value %u leaves the %zu spans", it, t, q, nb);
    }
    ++g_hostile;
  }
  return true;
}
}  // namespace

int main() {
  if (!honest() || !hostile()) return 1;
  std::printf("partytiles ok (%ld tables, %ld windows, %ld hostile)\n", g_tables, g_windows, g_hostile);
  return 0;
}
