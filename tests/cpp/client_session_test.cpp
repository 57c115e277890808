// client::ResponseSession (include/amphora.hpp over
// include/amphora_client_session.h): the parties' response texts handed in
// one by one, against KAT-3's structure, a host-computed round trip and the
// whole-call mirrors on the same texts.
//   KAT-3  amphora-java-client/.../SecretShareUtilTest.java:30-85
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>

#include "amphora.hpp"

using namespace amphora;

static int failures = 0;
#define EXPECT(c)                                                     \
  do {                                                                \
    if (!(c)) {                                                       \
      std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

static const u128 P = fromDecimal("198766463529478683931867765928436695041", ~(u128)0);
static const u128 R = fromDecimal("141515903391459779531506841503331516415", ~(u128)0);
static const u128 RI = fromDecimal("133854242216446749056083838363708373830", ~(u128)0);

// what() of the exception fn throws, "" if it throws none of type E
template <class E, class F>
static std::string thrown(F&& fn) {
  try {
    fn();
  } catch (const E& e) {
    return std::string("!") + e.what();
  }
  return "";
}

static std::vector<client::OdoText> textsOf(const Context& c, const std::vector<std::vector<Bytes>>& parts) {
  std::vector<client::OdoText> t(parts.size());
  for (size_t j = 0; j < parts.size(); ++j)
    for (int k = 0; k < 5; ++k) t[j].f[k] = wire::base64Encode(c, parts[j][k]);
  return t;
}

static void feed(client::ResponseSession& rs, const std::vector<client::OdoText>& texts,
                 const std::vector<int>& order) {
  for (int j : order) rs.addTexts(j, texts[j]);
}

static void run() {
  auto util = client::SecretShareUtil::of(P, R, RI);
  const Context& c = util.context();
  std::mt19937_64 rng(42);
  // KAT-3's structure as one party's response: w = s r, u = v r pass; w[last] - 10 fails
  auto nl = [&]() { return (u128)(rng() >> 1); };
  std::vector<u128> s, r, vv, w, u;
  for (int i = 0; i < 5; ++i) {
    s.push_back(nl()); r.push_back(nl()); vv.push_back(nl());
    w.push_back(s[i] * r[i] % P); u.push_back(vv[i] * r[i] % P);
  }
  {
    auto one = textsOf(c, {{c.toGfp(s), c.toGfp(r), c.toGfp(vv), c.toGfp(w), c.toGfp(u)}});
    client::ResponseSession rs(util, 1);
    rs.addTexts(0, one[0].f[0], one[0].f[1], one[0].f[2], one[0].f[3], one[0].f[4]);
    EXPECT(rs.words() == 5);
    EXPECT(rs.secrets() == s);
    w[4] = (w[4] + P - 10) % P;
    auto bad = textsOf(c, {{c.toGfp(s), c.toGfp(r), c.toGfp(vv), c.toGfp(w), c.toGfp(u)}});
    const std::string whole = thrown<IntegrityVerificationException>([&] { client::verifyOutputDeliveryText(util, bad); });
    client::ResponseSession rs2(util, 1);
    rs2.addTexts(0, bad[0]);
    const std::string mine = thrown<IntegrityVerificationException>([&] { rs2.secrets(); });
    EXPECT(whole.rfind("!Verification of secret has failed", 0) == 0);
    EXPECT(mine == whole);
  }
  // round trip: 3-party ODOs of secrets (w = s r mod p by a host double-and-add
  // ladder, independent of the kernels' Montgomery products)
  const size_t W = 385;
  const int N = 3;
  auto wide = [&]() { return ((u128)rng() << 64 | rng()) % P; };
  auto mulmod = [&](u128 a, u128 b) {
    u128 acc = 0;
    for (int bit = 127; bit >= 0; --bit) {
      acc = addMod(acc, acc, P);
      if ((b >> bit) & 1) acc = addMod(acc, a % P, P);
    }
    return acc;
  };
  std::vector<u128> vals[5];
  for (size_t i = 0; i < W; ++i) {
    const u128 y = wide(), rr = wide(), v = wide();
    vals[0].push_back(y); vals[1].push_back(rr); vals[2].push_back(v);
    vals[3].push_back(mulmod(y, rr)); vals[4].push_back(mulmod(v, rr));
  }
  std::vector<std::vector<Bytes>> parts(N, std::vector<Bytes>(5));
  for (int k = 0; k < 5; ++k) {
    std::vector<std::vector<u128>> sh(N, std::vector<u128>(W));
    for (size_t i = 0; i < W; ++i) {
      u128 rest = vals[k][i];
      for (int j = 0; j + 1 < N; ++j) {
        sh[j][i] = wide();
        rest = rest >= sh[j][i] ? rest - sh[j][i] : rest + (P - sh[j][i]);
      }
      sh[N - 1][i] = rest;
    }
    for (int j = 0; j < N; ++j) parts[j][k] = c.toGfp(sh[j]);
  }
  const auto texts = textsOf(c, parts);
  const std::vector<std::vector<int>> orders = {{0, 1, 2}, {2, 1, 0}, {1, 2, 0}};
  std::vector<u128> secrets(W);
  for (auto& x : secrets) x = rng();
  const auto wholeRecords = client::maskSecretText(util, secrets, texts);
  const auto wholeText = client::maskSecretDataText(util, secrets, texts);
  for (auto& order : orders) {
    {
      client::ResponseSession rs(util, N);
      feed(rs, texts, order);
      EXPECT(rs.secrets() == vals[0]);
    }
    {
      client::ResponseSession rs(util, N);
      feed(rs, texts, order);
      const auto rec = rs.maskSecretText(secrets);
      EXPECT(rec == wholeRecords);
      for (size_t i = 0; i < W; i += 97) {  // masked + mask == secret
        const u128 mv = c.fromGfp(wire::base64Decode(c, rec[i]))[0];
        EXPECT(addMod(mv, vals[0][i], P) == secrets[i] % P);
      }
    }
    {
      client::ResponseSession rs(util, N);
      feed(rs, texts, order);
      EXPECT(rs.maskSecretDataText(secrets) == wholeText);
    }
  }
  // a tampered w share: the whole call's exception and message, from the sums
  auto tampered = texts;
  {
    Bytes wt = parts[1][3];
    wt[16 * 192] ^= 1;
    tampered[1].f[3] = wire::base64Encode(c, wt);
  }
  const std::string wholeMsg = thrown<IntegrityVerificationException>([&] { client::verifyOutputDeliveryText(util, tampered); });
  EXPECT(wholeMsg.rfind("!Verification of secret has failed", 0) == 0);
  for (int fn = 0; fn < 3; ++fn) {
    client::ResponseSession rs(util, N);
    feed(rs, tampered, orders[fn]);
    EXPECT(thrown<IntegrityVerificationException>([&] {
             if (fn == 0) rs.secrets();
             else if (fn == 1) rs.maskSecretText(secrets);
             else rs.maskSecretDataText(secrets);
           }) == wholeMsg);
  }
  // bad characters in two parties: each reported when handed in, the smaller by the finish
  auto badChar = texts;
  badChar[2].f[0][7] = '*';
  badChar[1].f[2][100] = '!';
  const std::string wholeBad = thrown<AmphoraClientException>([&] { client::verifyOutputDeliveryText(util, badChar); });
  EXPECT(wholeBad.find("index 100 of party 1's vShares") != std::string::npos);
  {
    client::ResponseSession rs(util, N);
    EXPECT(thrown<AmphoraClientException>([&] { rs.addTexts(2, badChar[2]); })
               .find("index 7 of party 2's secretShares") != std::string::npos);
    rs.addTexts(0, badChar[0]);
    EXPECT(thrown<AmphoraClientException>([&] { rs.addTexts(1, badChar[1]); }) == wholeBad);
    EXPECT(thrown<AmphoraClientException>([&] { rs.secrets(); }) == wholeBad);
  }
  // unequal fields, another length than the first party's, a slot twice, a slot missing
  {
    client::ResponseSession rs(util, N);
    auto shortField = texts[1];
    shortField.f[2].resize(shortField.f[2].size() - 4);
    EXPECT(thrown<IllegalArgumentException>([&] { rs.addTexts(1, shortField); }) ==
           "!The provided shares must be of the same length");
    rs.addTexts(0, texts[0]);
    client::OdoText shorter;
    for (int k = 0; k < 5; ++k) shorter.f[k] = texts[1].f[k].substr(0, 64);
    EXPECT(thrown<IllegalArgumentException>([&] { rs.addTexts(1, shorter); }) ==
           "!The provided shares must be of the same length");
    EXPECT(!thrown<NativeError>([&] { rs.addTexts(0, texts[0]); }).empty());
    EXPECT(thrown<NativeError>([&] { rs.secrets(); }).find("party 1") != std::string::npos);
    rs.addTexts(2, texts[2]);
    rs.addTexts(1, texts[1]);  // the slot stayed open
    EXPECT(rs.secrets() == vals[0]);
    EXPECT(!thrown<NativeError>([&] { rs.secrets(); }).empty());  // a session finishes once
  }
  // more secret words than masks: a tampered mask set fails verification
  // first (DefaultAmphoraClient.java:153), an honest one the index check
  std::vector<u128> longer(secrets);
  longer.push_back(1);
  {
    client::ResponseSession rs(util, N);
    feed(rs, tampered, orders[1]);
    EXPECT(thrown<IntegrityVerificationException>([&] { rs.maskSecretText(longer); }) == wholeMsg);
    client::ResponseSession rs2(util, N);
    feed(rs2, texts, orders[2]);
    EXPECT(thrown<std::out_of_range>([&] { rs2.maskSecretDataText(longer); }) ==
           thrown<std::out_of_range>([&] { client::maskSecretDataText(util, longer, texts); }));
  }
}

int main() {
  try {
    run();
  } catch (const std::exception& e) {  // an exception no check expected: a failure, not an abort
    std::fprintf(stderr, "FAILED: uncaught %s\n", e.what());
    ++failures;
  }
  if (failures) {
    std::fprintf(stderr, "%d failure(s)\n", failures);
    return 1;
  }
  std::printf("client session mirror ok\n");
  return 0;
}
