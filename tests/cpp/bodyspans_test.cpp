// Stand-alone host driver of amphora_amd/csrc/bodyspans.hpp
// (tests/bodies/test_clients_bodies_cpu.py): the response-body scanner and the
// granule rule of the any-alignment accumulate kernel.  No library is linked.
//
//   bodyspans_test                 the built-in bodies and the granule rule against a
//                                  byte-by-byte enumeration; "clean" on success
//   bodyspans_test FILE            the catalogue FILE (below), then the same; "clean"
//   bodyspans_test scan FILE       one line per case: result and the ten numbers
//   bodyspans_test granules S N .. per pair "# S N first end", then "first n residue" per unit
//
// Every body is scanned from a heap buffer of EXACTLY its length, and so is
// every prefix of every body of at most 4,096 bytes (a cut string, a cut
// escape, a cut key): a read outside [body, body + len) is an ASan report.
//
// FILE: u32 count, then per case u32 len, the bytes, i32 expected result
// (a BodyScan value, or -1: any refusal), 5 u64 starts, 5 u64 lens
// (little-endian; starts / lens are compared only when 0 is expected).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "bodyspans.hpp"

namespace {
struct Case {
  std::string body;
  int expect;
  uint64_t starts[5], lens[5];
};

amph::BodyScan scan_exact(const std::string& b, size_t len, uint64_t* st, uint64_t* ln) {
  char* heap = (char*)std::malloc(len ? len : 1);  // exact size: no byte past the body exists
  std::memcpy(heap, b.data(), len);
  const amph::BodyScan r = amph::body_scan(len ? heap : heap + 1, len, st, ln);  // (len 0: a pointer with nothing behind it)
  std::free(heap);
  return r;
}

bool load(const char* path, std::vector<Case>& out) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  uint32_t n = 0;
  bool ok = std::fread(&n, 4, 1, f) == 1;
  for (uint32_t i = 0; ok && i < n; ++i) {
    Case c;
    uint32_t len = 0;
    int32_t e = 0;
    ok = std::fread(&len, 4, 1, f) == 1;
    c.body.resize(len);
    if (ok && len) ok = std::fread(&c.body[0], 1, len, f) == len;
    ok = ok && std::fread(&e, 4, 1, f) == 1 && std::fread(c.starts, 8, 5, f) == 5 && std::fread(c.lens, 8, 5, f) == 5;
    c.expect = e;
    if (ok) out.push_back(c);
  }
  std::fclose(f);
  return ok;
}

std::vector<Case> builtin() {
  std::vector<Case> v;
  auto plain = [&](const std::string& b) {
    Case c{b, 0, {}, {}};
    v.push_back(c);
  };
  auto refused = [&](const std::string& b, int why) {
    Case c{b, why, {}, {}};
    v.push_back(c);
  };
  const std::string five = "\"secretShares\":\"AAAA\",\"rShares\":\"BBBB\",\"vShares\":\"CCCC\",\"wShares\":\"DDDD\",\"uShares\":\"EEEE\"";
  plain("{" + five + "}");
  plain("{\"tags\":[{\"key\":\"rShares\",\"value\":\"a\\\"b\\\\\",\"x\":{\"uShares\":\"no\"}}], " + five + " }trailing\"");
  plain("{ \"secretShares\" :\n \"\",\"rShares\":\"\",\"vShares\":\"\",\"wShares\":\"\",\"uShares\":\"\"}");
  refused("", amph::kBodyNoObject);
  refused("[" + five + "]", amph::kBodyNoObject);
  refused("{\"secretShares\":\"AAAA\"}", amph::kBodyMissing);
  refused("{" + five + ",\"rShares\":\"BBBB\"}", amph::kBodyTwice);
  refused("{\"secretShares\":null," + five.substr(22) + "}", amph::kBodyNotString);
  refused("{\"secretShares\":\"AA\\/A\"," + five.substr(22) + "}", amph::kBodyEscape);
  refused("{" + five.substr(0, five.size() - 1), amph::kBodyUnterminated);
  refused("{\"k\":\"abc\\", amph::kBodyUnterminated);
  return v;
}

bool run(const std::vector<Case>& cases, const char* what) {
  for (size_t i = 0; i < cases.size(); ++i) {
    const Case& c = cases[i];
    uint64_t st[5] = {7, 7, 7, 7, 7}, ln[5] = {7, 7, 7, 7, 7};
    const amph::BodyScan r = scan_exact(c.body, c.body.size(), st, ln);
    const bool match = c.expect < 0 ? r != amph::kBodyOk : (int)r == c.expect;
    if (!match) {
      std::printf("%s case %zu: result %d (%s), expected %d\n", what, i, (int)r, amph::body_scan_reason(r), c.expect);
      return false;
    }
    if (r == amph::kBodyOk) {
      for (int k = 0; k < 5; ++k) {
        if (st[k] + ln[k] > c.body.size() || (st[k] == 0) || c.body[st[k] - 1] != '"' ||
            c.body[st[k] + ln[k]] != '"') {
          std::printf("%s case %zu: member %d [%llu, +%llu) is not a quoted span of the body\n", what, i, k,
                      (unsigned long long)st[k], (unsigned long long)ln[k]);
          return false;
        }
        if (c.expect == 0 && (c.starts[k] || c.lens[k]) && (st[k] != c.starts[k] || ln[k] != c.lens[k])) {
          std::printf("%s case %zu: member %d at %llu + %llu, expected %llu + %llu\n", what, i, k,
                      (unsigned long long)st[k], (unsigned long long)ln[k], (unsigned long long)c.starts[k],
                      (unsigned long long)c.lens[k]);
          return false;
        }
      }
    }
    if (c.body.size() <= 4096)  // every prefix: whatever the verdict, nothing past it is read
      for (size_t cut = 0; cut < c.body.size(); ++cut) (void)scan_exact(c.body, cut, st, ln);
  }
  return true;
}

// the granule rule against the text's bytes, one by one
bool granules_ok(uint64_t start, uint64_t nchars) {
  std::set<uint64_t> want;
  for (uint64_t i = 0; i < nchars; ++i) want.insert((start + i) >> 4);
  const amph::BodyGranules g = amph::body_granules(start, nchars);
  std::set<uint64_t> range, units;
  for (uint64_t x = g.first; x < g.end; ++x) range.insert(x);
  bool ok = range == want;
  for (uint64_t u = 0; u <= nchars / 16 + 1; ++u) {
    const amph::BodyUnit bu = amph::body_unit(start, nchars, u);
    std::set<uint64_t> mine;
    for (uint64_t i = 16 * u; i < 16 * u + 16 && i < nchars; ++i) mine.insert((start + i) >> 4);
    std::set<uint64_t> got;
    for (uint32_t x = 0; x < bu.n; ++x) got.insert(bu.first + x);
    ok = ok && got == mine && bu.n <= 2 && bu.residue == (start & 15) && bu.first == (start + 16 * u) >> 4;
    // a whole unit needs two granules exactly when the text does not start on one
    if (16 * u + 16 <= nchars) ok = ok && bu.n == ((start & 15) ? 2u : 1u);
    units.insert(got.begin(), got.end());
  }
  ok = ok && units == want;
  if (!ok) std::printf("granule rule: start %llu, nchars %llu\n", (unsigned long long)start, (unsigned long long)nchars);
  return ok;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc >= 4 && argc % 2 == 0 && !std::strcmp(argv[1], "granules")) {
    for (int a = 2; a + 1 < argc; a += 2) {
      const uint64_t start = std::strtoull(argv[a], nullptr, 10), nchars = std::strtoull(argv[a + 1], nullptr, 10);
      const amph::BodyGranules g = amph::body_granules(start, nchars);
      std::printf("# %llu %llu %llu %llu\n", (unsigned long long)start, (unsigned long long)nchars,
                  (unsigned long long)g.first, (unsigned long long)g.end);
      for (uint64_t u = 0; 16 * u < nchars + 16; ++u) {
        const amph::BodyUnit bu = amph::body_unit(start, nchars, u);
        std::printf("%llu %u %u\n", (unsigned long long)bu.first, bu.n, bu.residue);
      }
    }
    return 0;
  }
  if (argc == 3 && !std::strcmp(argv[1], "scan")) {
    std::vector<Case> cases;
    if (!load(argv[2], cases)) return 2;
    for (const Case& c : cases) {
      uint64_t st[5] = {0, 0, 0, 0, 0}, ln[5] = {0, 0, 0, 0, 0};
      const amph::BodyScan r = scan_exact(c.body, c.body.size(), st, ln);
      std::printf("%d", (int)r);
      for (int k = 0; k < 5 && r == amph::kBodyOk; ++k)
        std::printf(" %llu %llu", (unsigned long long)st[k], (unsigned long long)ln[k]);
      std::printf("\n");
    }
    return 0;
  }
  std::vector<Case> cases;
  if (argc == 2 && !load(argv[1], cases)) {
    std::printf("cannot read %s\n", argv[1]);
    return 2;
  }
  if (!run(builtin(), "built-in") || !run(cases, "catalogue")) return 1;
  for (uint64_t base : {0ull, 16ull, 4096ull + 32})
    for (uint64_t r = 0; r < 16; ++r)
      for (uint64_t around : {0ull, 16ull, 4096ull, 8192ull})
        for (uint64_t d = 0; d <= 40; ++d) {
          const uint64_t n = around + d >= 20 ? around + d - 20 : 0;
          if (!granules_ok(base + r, n)) return 1;
        }
  std::printf("clean: %zu built-in and %zu catalogue bodies, every prefix, the granule rule\n", builtin().size(),
              cases.size());
  return 0;
}
