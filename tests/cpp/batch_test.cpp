// Many secrets in one call, from C++ (tests/test_batch_calls_cpu.py,
// tests/test_batch_calls.py):
//   batch_test lookup        the segmented kernels' object lookup
//                            (amphora_amd/csrc/seglookup.hpp) compiled for the
//                            host, against a linear scan -- no GPU
//   batch_test gpu <file>    the gathered C ABI calls and the C++ mirror's
//                            batch functions over the batch in <file>, against
//                            the expected results stored with it (GPU)
// <file>, little-endian, written by the test from the C oracle:
//   u64 n_parties, K; 16 bytes each: prime, r, rInv; then per object
//   u64 W; i64 first_fail; [party][field] W words; W words expected secrets;
//   W words mask secrets; W words expected masked
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <random>

#include "amphora.hpp"
#include "seglookup.hpp"

#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                \
    }                                                              \
  } while (0)

namespace {

// every word of a table that keeps the contract: the owner by a linear scan
void check_table(const std::vector<uint64_t>& sizes) {
  std::vector<uint64_t> off(sizes.size() + 1, 0);
  for (size_t o = 0; o < sizes.size(); ++o) off[o + 1] = off[o] + sizes[o];
  // the table alone in its allocation: a read of offsets[n_objects + 1] would be out of bounds
  std::vector<uint64_t> exact(off);
  exact.shrink_to_fit();
  size_t owner = 0;
  for (uint64_t i = 0; i < off.back(); ++i) {
    while (!(off[owner] <= i && i < off[owner + 1])) ++owner;
    const size_t got = amph::seg_find(exact.data(), sizes.size(), i);
    if (got != owner) {
      std::fprintf(stderr, "word %llu of %zu objects: object %zu, expected %zu\n", (unsigned long long)i,
                   sizes.size(), got, owner);
      std::exit(1);
    }
  }
}

int lookup() {
  check_table({5});                               // a single object
  check_table({0, 0, 3, 1});                      // empty at the start (a run)
  check_table({2, 0, 4, 0, 0, 0, 1, 1, 0, 7});    // empty in the middle, alone and in a run
  check_table({3, 2, 0});                         // empty at the end
  check_table({4, 1, 0, 0, 0});                   // a run at the end
  check_table({0, 1, 0, 63, 64, 65, 1, 1, 1, 0, 130, 1025, 7, 0});  // the GPU tests' batch
  std::mt19937_64 rng(7);
  for (size_t n : {1, 2, 3, 64, 1000})
    for (int rep = 0; rep < 4; ++rep) {
      std::vector<uint64_t> sizes(n);
      for (auto& s : sizes) s = rep == 3 ? 1 : (rng() % 3 == 0 ? 0 : rng() % 9);  // a third empty
      if (rep == 1) sizes.front() = sizes.back() = 0;
      if (rep == 2) sizes.front() = sizes.back() = 5;
      check_table(sizes);
    }
  // tables that break the contract, and words past the end: the index stays in range
  for (size_t n : {1, 2, 3, 64, 1000})
    for (int rep = 0; rep < 8; ++rep) {
      std::vector<uint64_t> junk(n + 1);
      for (auto& x : junk) x = rep < 4 ? rng() : rng() % 50;  // unordered, offsets[0] != 0
      for (int q = 0; q < 200; ++q) {
        const uint64_t i = q < 100 ? rng() : rng() % 64;
        CHECK(amph::seg_find(junk.data(), n, i) < n);
      }
      CHECK(amph::seg_find(junk.data(), n, ~0ULL) < n);
      CHECK(amph::seg_find(junk.data(), n, 0) < n);
    }
  std::puts("lookup ok");
  return 0;
}

struct Object {
  uint64_t W = 0;
  int64_t ff = -1;
  std::vector<amphora::OutputDeliveryObject> odos;
  amphora::Bytes y, secrets, masked;
};

amphora::Bytes take(std::ifstream& in, size_t bytes) {
  amphora::Bytes b(bytes);
  in.read((char*)b.data(), (std::streamsize)bytes);
  CHECK(in.good() || bytes == 0);
  return b;
}
uint64_t take64(std::ifstream& in) {
  uint64_t x = 0;
  in.read((char*)&x, 8);
  CHECK(in.good());
  return x;
}

int gpu(const char* path) {
  using namespace amphora;
  std::ifstream in(path, std::ios::binary);
  CHECK(in.good());
  const uint64_t n = take64(in), K = take64(in);
  const Bytes p = take(in, 16), r = take(in, 16), ri = take(in, 16);
  std::vector<Object> obj(K);
  for (Object& o : obj) {
    o.W = take64(in);
    o.ff = (int64_t)take64(in);
    for (uint64_t j = 0; j < n; ++j) {
      Bytes f[5];
      for (auto& x : f) x = take(in, 16 * o.W);
      o.odos.emplace_back(f[0], f[1], f[2], f[3], f[4]);
    }
    o.y = take(in, 16 * o.W);
    o.secrets = take(in, 16 * o.W);
    o.masked = take(in, 16 * o.W);
  }
  auto util = client::SecretShareUtil::of(loadLe(p.data()), loadLe(r.data()), loadLe(ri.data()));

  // the C ABI: verdicts and words, also of the failed objects
  std::vector<amph_odo> v;
  std::vector<Bytes> outs, mouts;
  std::vector<uint8_t*> outp, moutp;
  std::vector<const uint8_t*> secp;
  std::vector<size_t> ns;
  bool any_fail = false;
  for (Object& o : obj) {
    for (auto& q : o.odos) v.push_back(q.view());
    outs.emplace_back(16 * o.W, 0xAA);
    mouts.emplace_back(16 * o.W, 0xAA);
    secp.push_back(o.secrets.data());
    ns.push_back(o.W);
    any_fail |= o.ff >= 0;
  }
  for (uint64_t o = 0; o < K; ++o) outp.push_back(outs[o].data()), moutp.push_back(mouts[o].data());
  std::vector<int64_t> ff(K, 77), mff(K, 77);
  int st = amph_recombine_verify_batch(util.context().get(), v.data(), (int)n, K, outp.data(), ff.data(), 0);
  CHECK(st == (any_fail ? AMPH_E_VERIFY : AMPH_OK));
  st = amph_mask_input_batch(util.context().get(), v.data(), (int)n, K, secp.data(), ns.data(), moutp.data(),
                             mff.data(), 0);
  CHECK(st == (any_fail ? AMPH_E_VERIFY : AMPH_OK));
  for (uint64_t o = 0; o < K; ++o) {
    CHECK(ff[o] == obj[o].ff);
    CHECK(mff[o] == obj[o].ff);
    CHECK(outs[o] == obj[o].y);
    CHECK(mouts[o] == obj[o].masked);
  }

  // the mirror: a value per honest secret, the reference's exception per failed one
  std::vector<std::vector<OutputDeliveryObject>> objects;
  std::vector<std::vector<u128>> secrets;
  for (Object& o : obj) {
    objects.push_back(o.odos);
    secrets.push_back(unpackWords(o.secrets));
  }
  const auto res = client::verifyOutputDeliveryObjectsBatch(util, objects);
  const auto mres = client::maskSecrets(util, secrets, objects);
  CHECK(res.size() == K && mres.size() == K);
  for (uint64_t o = 0; o < K; ++o) {
    if (obj[o].ff < 0) {
      CHECK(res[o].ok() && res[o].value == unpackWords(obj[o].y));
      CHECK(mres[o].ok() && mres[o].value.size() == obj[o].W);
      for (uint64_t i = 0; i < obj[o].W; ++i)
        CHECK(std::equal(mres[o].value[i].begin(), mres[o].value[i].end(), obj[o].masked.begin() + 16 * i));
      continue;
    }
    std::string single, batch, mbatch;
    try {
      client::verifyOutputDeliveryObjects(util, objects[o]);
    } catch (const IntegrityVerificationException& e) {
      single = e.what();
    }
    try {
      res[o].get();
    } catch (const IntegrityVerificationException& e) {
      batch = e.what();
    }
    try {
      mres[o].get();
    } catch (const IntegrityVerificationException& e) {
      mbatch = e.what();
    }
    CHECK(!single.empty() && batch == single && mbatch == single);
  }
  std::puts("gpu ok");
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc >= 2 && std::string(argv[1]) == "lookup") return lookup();
  if (argc >= 3 && std::string(argv[1]) == "gpu") return gpu(argv[2]);
  std::fprintf(stderr, "usage: batch_test lookup | gpu <file>\n");
  return 2;
}
