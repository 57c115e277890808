// Stand-alone host driver of amphora_amd/csrc/exchangetiles.hpp
// (tests/test_exchange_batch_cpu.py): which object's pairs an encode workgroup
// of the segmented exchange codec formats, and which object's text a decode
// workgroup parses.  No library is linked.
//
//   exchangetiles_test                 every check below, "exchangetiles ok" on success
//   exchangetiles_test tables NPAIRS TEXTS_LEN K p0..pK t0..t(K-1) l0..l(K-1)
//                                      one set of tables, contract or not: every
//                                      workgroup's tile and span must stay inside
//                                      the arrays; prints "inside" or the breach
//
// Honest tables, against a linear enumeration.  Encode: every workgroup w of
// the grid npairs / 256 + n_objects is looked up (xenc_tile); every pair has
// exactly one owner, in its own object; no tile holds pairs of two objects;
// an object's tiles are consecutive workgroups from base_tile, exactly one of
// them `first`; an object of no pairs has one tile of no pairs.  Decode: every
// span s of the grid texts_len / 8192 + 1 is looked up (xdec_span); every byte
// of every text lies in a span its object owns, at the right local index; a
// span of a gap or a slot's rest has no owner; an empty text owns one span.
// Hostile tables (decreasing, near 2^64, past the buffers, unaligned): no
// index outside [0, npairs], [0, texts_len] or [0, n_objects), and no stored
// character outside [0, out_cap).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "exchangetiles.hpp"

namespace {
long g_tables = 0, g_hostile = 0;

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return rng_state * 0x2545F4914F6CDD1Dull;
}

#define FAIL(...) return std::printf(__VA_ARGS__), std::printf("\n"), false

bool check_encode(const std::vector<uint64_t>& pairs, const char* what) {
  const size_t K = pairs.size();
  std::vector<uint64_t> poff(K + 1, 0);
  for (size_t o = 0; o < K; ++o) poff[o + 1] = poff[o] + pairs[o];
  const uint64_t T = poff[K];
  std::vector<uint8_t> owners(T, 0);
  std::vector<size_t> firsts(K, 0), tiles(K, 0);
  const size_t grid = amph::xenc_tile_grid(T, K);
  for (size_t w = 0; w < grid; ++w) {
    const amph::XEncTile t = amph::xenc_tile(poff.data(), K, T, w);
    if (t.object >= K) FAIL("%s: w %zu gives object %zu of %zu", what, w, t.object, K);
    if (t.base_tile + t.tiles > grid) FAIL("%s: w %zu: tiles [%zu, +%zu) leave the grid %zu", what, w, t.base_tile, t.tiles, grid);
    if (!t.owns) continue;
    const size_t o = t.object, local = w - t.base_tile;
    if (t.base_tile != poff[o] / 256 + o || t.tiles != (pairs[o] ? (pairs[o] + 255) / 256 : 1) || local >= t.tiles)
      FAIL("%s: w %zu: object %zu base %zu tiles %zu", what, w, o, t.base_tile, t.tiles);
    const uint64_t want0 = poff[o] + 256 * (uint64_t)local;
    const uint64_t wantn = pairs[o] - 256 * (uint64_t)local < 256 ? pairs[o] - 256 * (uint64_t)local : 256;
    if (t.pair0 != want0 || t.pairs != wantn || t.last != poff[o + 1] || t.first != (local == 0) ||
        (t.pairs == 0 && pairs[o] != 0))
      FAIL("%s: w %zu: pairs [%llu, +%u) last %llu first %d", what, w, (unsigned long long)t.pair0, t.pairs,
           (unsigned long long)t.last, (int)t.first);
    firsts[o] += t.first;
    ++tiles[o];
    for (uint64_t k = 0; k < t.pairs; ++k) {
      if (t.pair0 + k < poff[o] || t.pair0 + k >= poff[o + 1]) FAIL("%s: w %zu straddles two objects", what, w);
      if (++owners[t.pair0 + k] > 1) FAIL("%s: pair %llu has two owners", what, (unsigned long long)(t.pair0 + k));
    }
  }
  for (uint64_t k = 0; k < T; ++k)
    if (owners[k] != 1) FAIL("%s: pair %llu has no owner", what, (unsigned long long)k);
  for (size_t o = 0; o < K; ++o)
    if (firsts[o] != 1 || tiles[o] != (pairs[o] ? (pairs[o] + 255) / 256 : 1))
      FAIL("%s: object %zu: %zu first tiles, %zu tiles", what, o, firsts[o], tiles[o]);
  return true;
}

// lens[o] characters per text, gap[o] whole spans after object o's slot, tail characters after the last
bool check_decode(const std::vector<uint64_t>& lens, const std::vector<uint64_t>& pairs,
                  const std::vector<uint64_t>& gap, uint64_t tail, const char* what) {
  const size_t K = lens.size();
  std::vector<uint64_t> toff(K), poff(K + 1, 0);
  uint64_t at = 0;
  for (size_t o = 0; o < K; ++o) {
    toff[o] = at;
    const uint64_t slot = (lens[o] + 8191) / 8192 * 8192;
    at += (slot ? slot : 8192) + 8192 * gap[o];
    poff[o + 1] = poff[o] + pairs[o];
  }
  // the last text may end the buffer anywhere in its slot; an empty last text right at its end
  const uint64_t texts_len = K && tail == 0 ? toff[K - 1] + lens[K - 1] : at + tail;
  const size_t grid = amph::xdec_span_grid(texts_len);
  std::vector<long> owner(grid, -1);
  for (size_t o = 0; o < K; ++o) {
    const size_t n = lens[o] ? (size_t)((lens[o] + 8191) / 8192) : 1;
    for (size_t j = 0; j < n; ++j) {
      if (toff[o] / 8192 + j >= grid) FAIL("%s: object %zu's span %zu lies past the grid %zu", what, o, j, grid);
      owner[toff[o] / 8192 + j] = (long)o;
    }
  }
  for (size_t s = 0; s < grid; ++s) {
    const amph::XDecSpan d = amph::xdec_span(toff.data(), lens.data(), poff.data(), K, poff[K], texts_len, s);
    if (d.object >= K) FAIL("%s: span %zu gives object %zu of %zu", what, s, d.object, K);
    if (d.owns != (owner[s] >= 0)) FAIL("%s: span %zu owned %d, wanted %ld", what, s, (int)d.owns, owner[s]);
    if (!d.owns) continue;
    const size_t o = (size_t)owner[s];
    if (d.object != o || d.text0 != toff[o] || d.len != lens[o] || d.span0 != toff[o] / 8192 ||
        d.local != s - toff[o] / 8192 || d.spans != (lens[o] ? (lens[o] + 8191) / 8192 : 1) ||
        d.row0 != 2 * poff[o] || d.nvals != 2 * pairs[o] || d.span0 + d.spans > grid)
      FAIL("%s: span %zu: object %zu text [%llu, +%llu) local %zu of %zu rows %llu +%llu", what, s, d.object,
           (unsigned long long)d.text0, (unsigned long long)d.len, d.local, d.spans, (unsigned long long)d.row0,
           (unsigned long long)d.nvals);
  }
  ++g_tables;
  return true;
}

// any tables at all: every workgroup of both grids stays inside
bool inside(const std::vector<uint64_t>& poff, const std::vector<uint64_t>& toff, const std::vector<uint64_t>& lens,
            uint64_t npairs, uint64_t texts_len) {
  const size_t K = toff.size();
  size_t grid = amph::xenc_tile_grid(npairs, K);
  if (grid > 100000) grid = 100000;
  for (size_t w = 0; w < grid; ++w) {
    const amph::XEncTile t = amph::xenc_tile(poff.data(), K, npairs, w);
    const bool ok = t.object < K && t.pairs <= 256 && t.pair0 <= npairs && t.pairs <= npairs - t.pair0 &&
                    t.last <= npairs && (t.owns || (!t.pairs && !t.first)) && t.tiles >= 1 &&
                    t.base_tile + t.tiles <= amph::xenc_tile_grid(npairs, K) && (!t.owns || t.base_tile <= w);
    if (!ok) FAIL("w %zu: object %zu pairs [%llu, +%u) of %llu, tiles [%zu, +%zu)", w, t.object,
                  (unsigned long long)t.pair0, t.pairs, (unsigned long long)npairs, t.base_tile, t.tiles);
    // the stores: out_cap = texts_len, runs of every size a tile can have, anywhere in a text
    for (uint64_t into : {(uint64_t)0, (uint64_t)1, (uint64_t)23551, rnd(), ~(uint64_t)0, texts_len})
      for (uint64_t run : {(uint64_t)0, (uint64_t)13, (uint64_t)92 * 256}) {
        const uint64_t a = amph::xenc_store_at(toff[t.object], into, run, texts_len);
        if (a == ~(uint64_t)0) continue;
        // the '[' before, the run, the ']' after: all inside [0, out_cap)
        if (toff[t.object] >= texts_len || a < 1 || a + run < a || a + run >= texts_len || a != toff[t.object] + 1 + into)
          FAIL("w %zu: a run of %llu at %llu leaves the %llu characters", w, (unsigned long long)run,
               (unsigned long long)a, (unsigned long long)texts_len);
      }
  }
  size_t spans = amph::xdec_span_grid(texts_len);
  if (spans > 100000) spans = 100000;
  for (size_t s = 0; s < spans; ++s) {
    const amph::XDecSpan d = amph::xdec_span(toff.data(), lens.data(), poff.data(), K, npairs, texts_len, s);
    const bool ok = d.object < K && d.text0 % 8192 == 0 && d.text0 <= texts_len && d.len <= texts_len - d.text0 &&
                    d.spans >= 1 && d.span0 + d.spans <= amph::xdec_span_grid(texts_len) &&
                    (!d.owns || (d.local < d.spans && d.span0 + d.local == s)) && d.row0 % 2 == 0 &&
                    d.row0 / 2 <= npairs && d.nvals / 2 <= npairs - d.row0 / 2;
    if (!ok) FAIL("span %zu: object %zu text [%llu, +%llu) of %llu, rows [%llu, +%llu) of %llu", s, d.object,
                  (unsigned long long)d.text0, (unsigned long long)d.len, (unsigned long long)texts_len,
                  (unsigned long long)d.row0, (unsigned long long)d.nvals, (unsigned long long)(2 * npairs));
  }
  ++g_hostile;
  return true;
}

const uint64_t kPairs[] = {0, 1, 2, 255, 256, 257, 0, 513, 1024, 0};
const uint64_t kLens[] = {0, 2, 15, 8191, 8192, 8193, 16384, 0, 16385, 30000, 2};
constexpr size_t kNP = sizeof(kPairs) / sizeof(kPairs[0]), kNL = sizeof(kLens) / sizeof(kLens[0]);

bool honest() {
  if (!check_encode(std::vector<uint64_t>(kPairs, kPairs + kNP), "suite sizes")) return false;
  for (uint64_t g : {(uint64_t)0, (uint64_t)1, (uint64_t)3})
    for (uint64_t tail : {(uint64_t)0, (uint64_t)1, (uint64_t)8192, (uint64_t)8193}) {
      std::vector<uint64_t> l(kLens, kLens + kNL), p(kNL);
      for (size_t o = 0; o < kNL; ++o) p[o] = kPairs[o % kNP];
      if (!check_decode(l, p, std::vector<uint64_t>(kNL, g), tail, "suite lengths")) return false;
    }
  for (size_t K : {(size_t)1, (size_t)2, (size_t)3, (size_t)64, (size_t)300})
    for (size_t shift = 0; shift < kNL; ++shift) {
      std::vector<uint64_t> p(K), l(K), g(K);
      for (size_t o = 0; o < K; ++o) {
        p[o] = kPairs[(o + shift) % kNP];
        l[o] = kLens[(o + shift) % kNL];
        g[o] = (o + shift) % 3;
      }
      if (!check_encode(p, "cycle") || !check_decode(l, p, g, shift % 2 ? 8192 * shift + 5 : 0, "cycle")) return false;
      if (!check_encode(std::vector<uint64_t>(K, kPairs[shift % kNP]), "uniform")) return false;
      if (!check_decode(std::vector<uint64_t>(K, kLens[shift]), p, std::vector<uint64_t>(K, 0), 0, "uniform"))
        return false;
    }
  for (int it = 0; it < 3000; ++it) {
    const size_t K = 1 + rnd() % 24;
    std::vector<uint64_t> p(K), l(K), g(K);
    for (size_t o = 0; o < K; ++o) {
      const uint64_t r = rnd() % 8;
      p[o] = r < 2 ? 0 : r < 4 ? kPairs[rnd() % kNP] : r < 7 ? rnd() % 800 : 1000 + rnd() % 3000;
      const uint64_t q = rnd() % 8;
      l[o] = q < 1 ? 0 : q < 4 ? kLens[rnd() % kNL] : rnd() % 40000;
      g[o] = rnd() % 3;
    }
    if (!check_encode(p, "random") || !check_decode(l, p, g, rnd() % 2 ? rnd() % 20000 : 0, "random")) return false;
  }
  return true;
}

uint64_t hostile_value(uint64_t a, uint64_t b) {
  switch (rnd() % 8) {
    case 0: return ~(uint64_t)0 - rnd() % 5000;
    case 1: return ((uint64_t)1 << 63) + rnd() % 5000 - 2500;
    case 2: return a + rnd() % 400;
    case 3: return b + rnd() % 9000;
    case 4: return b - (b ? rnd() % (b < 9000 ? b : 9000) : 0);
    case 5: return rnd();
    default: return rnd() % (a + 200);
  }
}

bool hostile() {
  for (int it = 0; it < 10000; ++it) {
    const size_t K = 1 + rnd() % 12;
    const uint64_t npairs = it % 50 == 0 ? ((uint64_t)1 << 40) + rnd() % 1000 : rnd() % 3000;
    const uint64_t texts_len = it % 70 == 0 ? ((uint64_t)1 << 44) + rnd() % 8192 : rnd() % 200000;
    std::vector<uint64_t> poff(K + 1), toff(K), lens(K);
    for (auto& x : poff) x = hostile_value(npairs, texts_len);
    for (auto& x : toff) x = hostile_value(npairs, texts_len);
    for (auto& x : lens) x = hostile_value(npairs, texts_len);
    if (it % 3 == 0) {  // an honest pair table under hostile slots, and the other way round
      poff[0] = 0;
      for (size_t o = 0; o < K; ++o) poff[o + 1] = poff[o] + rnd() % 400;
    }
    if (it % 3 == 1)
      for (size_t o = 0; o < K; ++o) toff[o] = 8192 * (rnd() % 30);
    if (!inside(poff, toff, lens, npairs, texts_len)) {
      std::printf("hostile table %d breaks out\n", it);
      return false;
    }
  }
  return true;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc > 4 && !std::strcmp(argv[1], "tables")) {
    const uint64_t npairs = std::strtoull(argv[2], nullptr, 10), texts_len = std::strtoull(argv[3], nullptr, 10);
    const size_t K = std::strtoull(argv[4], nullptr, 10);
    if (K == 0 || (size_t)argc != 5 + 3 * K + 1)
      return std::printf("usage: tables NPAIRS TEXTS_LEN K p0..pK t0..t(K-1) l0..l(K-1)\n"), 2;
    std::vector<uint64_t> poff(K + 1), toff(K), lens(K);
    for (size_t i = 0; i <= K; ++i) poff[i] = std::strtoull(argv[5 + i], nullptr, 10);
    for (size_t i = 0; i < K; ++i) toff[i] = std::strtoull(argv[6 + K + i], nullptr, 10);
    for (size_t i = 0; i < K; ++i) lens[i] = std::strtoull(argv[6 + 2 * K + i], nullptr, 10);
    if (!inside(poff, toff, lens, npairs, texts_len)) return 1;
    std::printf("inside\n");
    return 0;
  }
  if (!honest() || !hostile()) return 1;
  std::printf("exchangetiles ok (%ld tables, %ld hostile)\n", g_tables, g_hostile);
  return 0;
}
