// C ABI of libamphora_hip (declared in include/amphora_client_bodies.h): a
// party's K response bodies handed to the K-secret client session
// (clients_session.hip) as they lie in memory.  amph_bodies_scan finds the
// five members of one body (bodyspans.hpp, host code); the party calls give
// k_acc_b64's any-alignment form ONE buffer and a table starts[5][K] of byte
// starts, one launch per party whatever K is.
//
// Host mode builds ONE image (BatchImage, as amph_clients_party): the starts
// table, then every present body copied whole to a multiple of 16, so each
// granule the kernel loads lies inside the image.  Device mode writes the
// table into the session's page-locked image of that party slot and uploads
// it by one hipMemcpyAsync in front of the launch; the device table is
// rewritten in stream order, the host image of a slot is written once.
#include "bodyspans.hpp"
#include "capi_internal.hpp"

namespace {
inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

// what both party calls check before anything is launched (c->mu held)
int bodies_slot_check(amph_clients* p, int party, const uint64_t* starts) {
  if (!starts) return fail(AMPH_E_PARAM, "null starts");
  if (party < 0 || party >= p->n)
    return fail(AMPH_E_PARAM, "party must be in [0, " + std::to_string(p->n - 1) + "]");
  if (p->have >> party & 1u) return fail(AMPH_E_PARAM, "party " + std::to_string(party) + "'s slot is already taken");
  return AMPH_OK;
}

bool body_absent(const uint64_t* five) {
  for (int k = 0; k < 5; ++k)
    if (five[k] == AMPH_BODY_ABSENT) return true;
  return false;
}

// object o's five starts against the `room` bytes they index
int bodies_fit(const amph_clients* p, size_t o, const uint64_t* five, size_t room) {
  const size_t nc = amph::wire_text_chars(p->woff[o + 1] - p->woff[o]);
  for (int k = 0; k < 5; ++k)
    if (five[k] > room || nc > room - five[k])
      return fail(AMPH_E_PARAM, "object " + std::to_string(o) + ": " + kOdoFieldNames[k] + " starts at byte " +
                                    std::to_string(five[k]) + ", its " + std::to_string(nc) +
                                    " characters end past the " + std::to_string(room) + " bytes given");
  return AMPH_OK;
}
}  // namespace

extern "C" {

int amph_bodies_scan(const char* body, size_t len, uint64_t starts[5], uint64_t lens[5]) {
  if (!body || !starts || !lens) return fail(AMPH_E_PARAM, "null body, starts or lens");
  uint64_t st[5], ln[5];
  const amph::BodyScan r = amph::body_scan(body, len, st, ln);
  if (r != amph::kBodyOk)
    return fail(AMPH_E_PARAM, std::string("not a plain response body: ") + amph::body_scan_reason(r));
  std::copy(st, st + 5, starts);
  std::copy(ln, ln + 5, lens);
  return AMPH_OK;
}

int amph_bodies_party(amph_clients* p, int party, const char* const* bodies, const size_t* body_lens,
                      const uint64_t* starts) {
  if (int st = clients_check(p, false, true)) return st;
  amph_ctx* c = p->c;
  const size_t K = p->K, T = p->T;
  HIP_TRY(use_device(c->device));
  std::unique_lock<std::mutex> g(c->mu);
  if (int st = bodies_slot_check(p, party, starts)) return st;
  if (!bodies || !body_lens) return fail(AMPH_E_PARAM, "null bodies or body_lens");
  std::vector<uint64_t> at(K, 0);  // where each present body lies in the image's text region
  size_t total = 0;
  for (size_t o = 0; o < K; ++o) {
    if (body_absent(starts + 5 * o)) continue;
    if (!bodies[o] && body_lens[o]) return fail(AMPH_E_PARAM, "object " + std::to_string(o) + ": null body");
    if (int st = bodies_fit(p, o, starts + 5 * o, body_lens[o])) return st;
    at[o] = total;
    total += align16(body_lens[o]);
  }
  if (T == 0) {
    p->have |= 1u << party;
    return AMPH_OK;
  }
  BatchImage m;
  m.lock = std::move(g);
  const size_t tab = m.in(40 * K), txt = m.in(total);
  m.verdicts(K, "verdict array");
  if (int st = m.open(c, &amph_ctx::clients_copies, "clients")) return st;
  uint64_t* table = (uint64_t*)m.host(tab);  // starts[5][K], rebased on the text region
  for (size_t o = 0; o < K; ++o) {
    const bool absent = body_absent(starts + 5 * o);
    if (!absent && body_lens[o]) std::memcpy(m.host(txt + at[o]), bodies[o], body_lens[o]);  // the body, whole
    for (int k = 0; k < 5; ++k) table[k * K + o] = absent ? AMPH_BODY_ABSENT : at[o] + starts[5 * o + k];
  }
  if (int st = m.upload()) return st;
  const hipError_t e =
      amph::launch_acc_b64_bodies((const char*)m.dev(txt), party, p->d_woff, m.dev_table(tab), K,
                                  amph::wire_tile_grid(T, K), p->sums, p->d_bad, m.dverd, c->f, cfg(c, m.s, T));
  if (e == hipSuccess) p->have |= 1u << party;  // the sums hold this party from here on, whatever its verdict
  if (int st = m.finish(e, "k_acc_b64")) return st;
  const unsigned long long* got = m.verdict_words();
  std::vector<unsigned long long> v(K, amph::kNoFail);  // (no MAC verdicts in a party call)
  v.insert(v.end(), got, got + K);
  for (size_t o = 0; o < K; ++o)
    if (got[o] < p->bad_host[o]) p->bad_host[o] = got[o];
  std::vector<int64_t> none(K), bad(K);
  return wire_batch_status(v.data(), K, p->woff.data(), none.data(), bad.data());
}

int amph_bodies_party_dev(amph_clients* p, int party, const char* buffer, size_t nbytes, const uint64_t* starts,
                          void* stream) {
  if (int st = clients_check(p, true, true)) return st;
  if (int st = check_dev_words({buffer})) return st;
  amph_ctx* c = p->c;
  hipStream_t s = (hipStream_t)stream;
  const size_t K = p->K;
  HIP_TRY(use_device(c->device));
  std::lock_guard<std::mutex> g(c->mu);
  if (int st = bodies_slot_check(p, party, starts)) return st;
  if (!buffer && p->T) return fail(AMPH_E_PARAM, "null buffer");
  for (size_t o = 0; o < K; ++o)
    if (!body_absent(starts + 5 * o))
      if (int st = bodies_fit(p, o, starts + 5 * o, nbytes)) return st;
  p->dstream = s;
  if (p->T) {
    uint64_t* table = p->starts_host + (size_t)party * 5 * K;  // this slot's image: written once
    for (size_t o = 0; o < K; ++o) {
      const bool absent = body_absent(starts + 5 * o);
      for (int k = 0; k < 5; ++k) table[k * K + o] = absent ? AMPH_BODY_ABSENT : starts[5 * o + k];
    }
    HIP_TRY(hipMemcpyAsync(p->d_starts, table, 40 * K, hipMemcpyHostToDevice, s));
    const hipError_t e =
        amph::launch_acc_b64_bodies(buffer, party, p->d_woff, p->d_starts, K, amph::wire_tile_grid(p->T, K),
                                    p->sums, p->d_bad, nullptr, c->f, cfg(c, s, p->T));
    if (e != hipSuccess) return hip_fail(e, "k_acc_b64");
  }
  p->have |= 1u << party;
  return AMPH_OK;
}

}  // extern "C"
