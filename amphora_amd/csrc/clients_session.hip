// C ABI of libamphora_hip (declared in include/amphora_client_batch.h): the
// client side as a session for K secrets -- each party's five slotted field
// buffers are added into running sums packed on the word table (k_acc_b64's
// segmented form, one launch per party whatever K is), and the finish calls
// run K_RV over the sums (k_rv_seg, the sums as a one-party ODO) or K_MASK
// from them (k_mask_sums_seg) with one verdict per object.
//
// Device memory: one pooled buffer (the party sessions' pool) carved into the
// five sums, the three offset tables (word, field text, framed text) and the
// session's K bad-character words.  Host mode moves a party's K texts, and the
// finish call's secrets and outputs, as ONE image each (BatchImage: the
// small-call arena in place, or one blocking copy each way while the
// context's stream is idle -- kPageableRule), counted in amph_clients_copies.
// Every launch of a host session goes on the context's first stream under the
// context's mutex, every launch of a device session on the caller's stream, so
// the read-modify-write on the sums runs in order.  Device mode uploads the
// tables by one hipMemcpyAsync from a page-locked image the session owns.
#include "capi_internal.hpp"

// (struct amph_clients: capi_internal.hpp -- clients_bodies.hip works on the same session)
namespace capi {
int clients_check(amph_clients* p, bool dev, bool open) {
  if (!p || !p->c) return fail(AMPH_E_PARAM, "null client batch session");
  if (p->dev != dev)
    return fail(AMPH_E_PARAM, dev ? "a host-mode client batch session takes the host calls"
                                  : "a device-mode client batch session takes the *_dev calls");
  if (open && p->finished) return fail(AMPH_E_PARAM, "the client batch session is already finished");
  return AMPH_OK;
}
}  // namespace capi

namespace {
size_t clients_table_bytes(size_t K) { return 8 * (3 * K + 1); }

int clients_all_in(const amph_clients* p) {
  for (int j = 0; j < p->n; ++j)
    if (!(p->have >> j & 1u)) return fail(AMPH_E_PARAM, "party " + std::to_string(j) + "'s texts are missing");
  return AMPH_OK;
}

int verdicts_misaligned(std::initializer_list<const void*> ptrs) {
  for (const void* q : ptrs)
    if ((uintptr_t)q & 7) return fail(AMPH_E_PARAM, "device verdict arrays and records must be 8-byte aligned");
  return AMPH_OK;
}

int clients_begin(amph_ctx* c, const uint64_t* woff, size_t K, int n_parties, bool dev, hipStream_t stream,
                  amph_clients** out) {
  if (!out) return fail(AMPH_E_PARAM, "null session output");
  *out = nullptr;
  if (check_ctx(c)) return AMPH_E_PARAM;
  if (K == 0) return fail(AMPH_E_PARAM, "a client batch session needs at least one object");
  if (!woff) return fail(AMPH_E_PARAM, "null word_offsets");
  if (n_parties < 1 || n_parties > AMPH_MAX_PARTIES) return fail(AMPH_E_PARAM, "n_parties must be in [1, 16]");
  if (woff[0] != 0) return fail(AMPH_E_PARAM, "word_offsets[0] must be 0");
  for (size_t o = 0; o < K; ++o)
    if (woff[o + 1] < woff[o])
      return fail(AMPH_E_PARAM, "word_offsets must be nondecreasing (object " + std::to_string(o) + ")");
  if (woff[K] > ((uint64_t)1 << 40)) return fail(AMPH_E_PARAM, "too many words");
  if (dev && !c->sub.empty()) return fail(AMPH_E_PARAM, "device-mode sessions need a single-device context");
  c = first_device(c);  // a multi-device context runs sessions on its first device
  HIP_TRY(use_device(c->device));
  std::lock_guard<std::mutex> g(c->mu);
  std::unique_ptr<amph_clients> p(new amph_clients);
  p->c = c;
  p->K = K;
  p->T = (size_t)woff[K];
  p->n = n_parties;
  p->dev = dev;
  p->woff.assign(woff, woff + K + 1);
  p->foff.resize(K);
  p->uoff.resize(K);
  for (size_t o = 0; o < K; ++o) {
    const size_t W = (size_t)(woff[o + 1] - woff[o]);
    p->foff[o] = p->field_chars;
    p->uoff[o] = p->upload_chars;
    p->used_chars = p->field_chars + amph::wire_text_chars(W);
    p->field_chars += amph::wire_slot_chars(W);
    p->upload_chars += amph::upload_slot_chars(W);
  }
  if (!dev) p->bad_host.assign(K, amph::kNoFail);
  if (dev) p->dstream = stream;
  else if (int st = host_stream(c, 0, &p->dstream)) return st;
  const size_t field = align256(16 * p->T), tab = align256(clients_table_bytes(K));
  // (behind the verdict words: the body calls' starts[5][K], device mode -- include/amphora_client_bodies.h)
  if (pool_ensure(c, p->mem, 5 * field + tab + align256(8 * K) + (dev ? align256(40 * K) : 0)) != hipSuccess)
    return fail(AMPH_E_NOMEM, "client batch session device memory");
  uint8_t* base = (uint8_t*)p->mem.p;
  for (int k = 0; k < 5; ++k) p->sums.s[k] = (uint4*)(base + k * field);
  p->d_woff = (uint64_t*)(base + 5 * field);
  p->d_foff = p->d_woff + K + 1;
  p->d_uoff = p->d_foff + K;
  p->d_bad = (unsigned long long*)(base + 5 * field + tab);
  if (dev) p->d_starts = (uint64_t*)(base + 5 * field + tab + align256(8 * K));
  std::vector<uint64_t> img(clients_table_bytes(K) / 8);
  std::copy(p->woff.begin(), p->woff.end(), img.begin());
  std::copy(p->foff.begin(), p->foff.end(), img.begin() + K + 1);
  std::copy(p->uoff.begin(), p->uoff.end(), img.begin() + 2 * K + 1);
  hipError_t e = hipSuccess;
  if (dev) {
    // (after the tables: one starts[5][K] image per party slot for the body calls)
    if (p->tables_host.ensure(clients_table_bytes(K) + (size_t)n_parties * 40 * K) != hipSuccess) {
      pool_put(c, p->mem);
      return fail(AMPH_E_NOMEM, "client batch session page-locked tables");
    }
    std::memcpy(p->tables_host.p, img.data(), clients_table_bytes(K));
    p->starts_host = (uint64_t*)((uint8_t*)p->tables_host.p + clients_table_bytes(K));
    e = hipMemcpyAsync(p->d_woff, p->tables_host.p, clients_table_bytes(K), hipMemcpyHostToDevice, p->dstream);
  } else {
    // the context's stream is idle between host calls (kPageableRule)
    e = hipStreamSynchronize(p->dstream);
    if (e == hipSuccess) e = hipMemcpy(p->d_woff, img.data(), clients_table_bytes(K), hipMemcpyHostToDevice);
  }
  if (e == hipSuccess && p->T) e = hipMemsetAsync(base, 0, 5 * field, p->dstream);
  if (e == hipSuccess) e = hipMemsetAsync(p->d_bad, 0x7F, 8 * K, p->dstream);
  if (e == hipSuccess && !dev) e = hipStreamSynchronize(p->dstream);
  if (e != hipSuccess) {  // the upload may be in flight: its source is freed only after the stream
    (void)hipStreamSynchronize(p->dstream);
    pool_put(c, p->mem);
    return hip_fail(e, "client batch session tables and sums");
  }
  *out = p.release();
  return AMPH_OK;
}

// what every party call checks before anything is launched (c->mu held)
int clients_slot_check(amph_clients* p, int party, const amph_odo_b64* texts) {
  if (!texts) return fail(AMPH_E_PARAM, "null texts");
  if (party < 0 || party >= p->n)
    return fail(AMPH_E_PARAM, "party must be in [0, " + std::to_string(p->n - 1) + "]");
  if (p->have >> party & 1u) return fail(AMPH_E_PARAM, "party " + std::to_string(party) + "'s slot is already taken");
  if (texts->nchars < p->used_chars)
    return fail(AMPH_E_LEN, "party " + std::to_string(party) + ": field buffers of " + std::to_string(texts->nchars) +
                                " characters, the last of the " + std::to_string(p->K) + " texts ends at " +
                                std::to_string(p->used_chars));
  for (int k = 0; k < 5 && p->T; ++k)
    if (!b64_field(*texts, k)) return fail(AMPH_E_PARAM, "null ODO field text");
  return AMPH_OK;
}

amph::OdoSet clients_odo(const amph_clients* p) {  // the sums as a one-party ODO of canonical words
  amph::OdoSet o{};
  for (int k = 0; k < 5; ++k) o.f[k][0] = p->sums.s[k];
  return o;
}

// the finish calls' arguments, either mode (before the device is touched)
int clients_finish_args(amph_clients* p, bool dev, const uint8_t* out_y, const uint8_t* secrets, const char* out_text,
                        size_t out_cap, bool mask, bool json, const int64_t* first_fails, const int64_t* bad_chars) {
  if (int st = clients_check(p, dev, true)) return st;
  if (!first_fails || !bad_chars) return fail(AMPH_E_PARAM, "null verdict array");
  if (!mask && p->T && !out_y) return fail(AMPH_E_PARAM, "null output");
  if (mask && p->T && !secrets) return fail(AMPH_E_PARAM, "null secrets");
  if (json && !out_text) return fail(AMPH_E_PARAM, "null output text");
  if (json && out_cap < p->upload_chars)
    return fail(AMPH_E_LEN, "output capacity " + std::to_string(out_cap) + " below the " +
                                std::to_string(p->upload_chars) + " characters of the " + std::to_string(p->K) +
                                " framed texts");
  return AMPH_OK;
}

// Host mode of the finish calls: verify (out_y) or mask (the other outputs).
int clients_finish_host(amph_clients* p, uint8_t* out_y, const uint8_t* secrets, uint8_t* out16, char* out24,
                        char* out_text, size_t out_cap, bool mask, bool json, int64_t* first_fails,
                        int64_t* bad_chars) {
  if (int st = clients_finish_args(p, false, out_y, secrets, out_text, out_cap, mask, json, first_fails, bad_chars))
    return st;
  amph_ctx* c = p->c;
  const size_t K = p->K, T = p->T;
  HIP_TRY(use_device(c->device));
  std::unique_lock<std::mutex> g(c->mu);
  if (int st = clients_all_in(p)) return st;
  for (size_t o = 0; o < K; ++o) first_fails[o] = bad_chars[o] = -1;
  p->finished = true;
  if (T == 0) {  // every object is empty: nothing to verify, every framed text is "[]"
    for (size_t o = 0; json && o < K; ++o) std::memcpy(out_text + p->uoff[o], "[]", 2);
    return AMPH_OK;
  }
  if (!mask) out16 = out_y;
  BatchImage m;
  m.lock = std::move(g);
  const size_t sec = m.in(mask ? 16 * T : 0);
  const size_t o16 = m.out(out16 ? 16 * T : 0), o24 = m.out(out24 ? 24 * T : 0);
  const size_t otx = m.out(json ? p->upload_chars : 0);
  m.verdicts(K, "verdict array");
  if (int st = m.open(c, &amph_ctx::clients_copies, "clients")) return st;
  if (mask) std::memcpy(m.host(sec), secrets, 16 * T);
  if (int st = m.upload()) return st;
  const amph::LaunchCfg lc = cfg(c, m.s, T);
  const hipError_t e =
      mask ? amph::launch_mask_sums_seg(p->sums, p->d_woff, p->d_uoff, K, amph::wire_tile_grid(T, K),
                                        (const uint4*)m.dev(sec), out16 ? (uint4*)m.dev(o16) : nullptr,
                                        out24 ? (char*)m.dev(o24) : nullptr, json ? (char*)m.dev(otx) : nullptr,
                                        m.dverd, c->f, lc)
           : amph::launch_recombine_verify_seg(clients_odo(p), 1, T, (uint4*)m.dev(o16), m.dverd, p->d_woff, K, 0,
                                               c->f, lc);
  if (int st = m.finish(e, mask ? "k_mask_sums_seg" : "k_rv_seg")) return st;
  if (out16) std::memcpy(out16, m.host(o16), 16 * T);
  if (out24) std::memcpy(out24, m.host(o24), 24 * T);
  for (size_t o = 0; json && o < K; ++o)  // text by text: the caller's gaps stay untouched
    std::memcpy(out_text + p->uoff[o], m.host(otx + p->uoff[o]),
                amph::masked_input_data_chars(p->woff[o + 1] - p->woff[o]));
  std::vector<unsigned long long> v(m.verdict_words(), m.verdict_words() + K);
  v.insert(v.end(), p->bad_host.begin(), p->bad_host.end());
  return wire_batch_status(v.data(), K, p->woff.data(), first_fails, bad_chars);
}

// Device mode of the finish calls.
int clients_finish_dev(amph_clients* p, uint8_t* out_y, const uint8_t* secrets, uint8_t* out16, char* out24,
                       char* out_text, size_t out_cap, bool mask, bool json, int64_t* first_fails, int64_t* bad_chars,
                       hipStream_t s) {
  if (int st = clients_finish_args(p, true, out_y, secrets, out_text, out_cap, mask, json, first_fails, bad_chars))
    return st;
  if (int st = check_dev_words({out_y, secrets, out16, out_text})) return st;
  if (int st = verdicts_misaligned({out24, first_fails, bad_chars})) return st;
  amph_ctx* c = p->c;
  const size_t K = p->K, T = p->T;
  HIP_TRY(use_device(c->device));
  std::lock_guard<std::mutex> g(c->mu);
  if (int st = clients_all_in(p)) return st;
  p->dstream = s;
  p->finished = true;
  HIP_TRY(hipMemsetAsync(first_fails, 0x7F, 8 * K, s));
  // the session's K bad-character words: the one operation besides the launch
  HIP_TRY(hipMemcpyAsync(bad_chars, p->d_bad, 8 * K, hipMemcpyDeviceToDevice, s));
  if (T == 0 && !json) return AMPH_OK;  // (the framed launch runs: every object gets its "[]")
  const amph::LaunchCfg lc = cfg(c, s, T);
  const hipError_t e =
      mask ? amph::launch_mask_sums_seg(p->sums, p->d_woff, p->d_uoff, K, amph::wire_tile_grid(T, K),
                                        (const uint4*)secrets, (uint4*)out16, out24, json ? out_text : nullptr,
                                        (unsigned long long*)first_fails, c->f, lc)
           : amph::launch_recombine_verify_seg(clients_odo(p), 1, T, (uint4*)out_y, (unsigned long long*)first_fails,
                                               p->d_woff, K, 0, c->f, lc);
  return e == hipSuccess ? AMPH_OK : hip_fail(e, mask ? "k_mask_sums_seg" : "k_rv_seg");
}
}  // namespace

extern "C" {

int amph_clients_begin(amph_ctx* c, const uint64_t* word_offsets, size_t n_objects, int n_parties,
                       amph_clients** out) {
  return clients_begin(c, word_offsets, n_objects, n_parties, false, nullptr, out);
}

int amph_clients_begin_dev(amph_ctx* c, const uint64_t* word_offsets, size_t n_objects, int n_parties, void* stream,
                           amph_clients** out) {
  return clients_begin(c, word_offsets, n_objects, n_parties, true, (hipStream_t)stream, out);
}

int amph_clients_party(amph_clients* p, int party, const amph_odo_b64* texts, int64_t* bad_chars) {
  if (int st = clients_check(p, false, true)) return st;
  amph_ctx* c = p->c;
  const size_t K = p->K, T = p->T;
  HIP_TRY(use_device(c->device));
  std::unique_lock<std::mutex> g(c->mu);
  if (int st = clients_slot_check(p, party, texts)) return st;
  for (size_t o = 0; bad_chars && o < K; ++o) bad_chars[o] = -1;
  if (T == 0) {
    p->have |= 1u << party;
    return AMPH_OK;
  }
  BatchImage m;
  m.lock = std::move(g);
  const size_t fchars = align256(p->used_chars);
  const size_t txt = m.in(5 * fchars);
  m.verdicts(K, "verdict array");
  if (int st = m.open(c, &amph_ctx::clients_copies, "clients")) return st;
  amph::TextSet tx{};
  for (int k = 0; k < 5; ++k) {  // text by text: what lies between them is never read
    const char* src = b64_field(*texts, k);
    for (size_t o = 0; o < K; ++o)
      if (const size_t nc = amph::wire_text_chars(p->woff[o + 1] - p->woff[o]))
        std::memcpy(m.host(txt + k * fchars + p->foff[o]), src + p->foff[o], nc);
    tx.t[k][0] = (const char*)m.dev(txt + k * fchars);
  }
  if (int st = m.upload()) return st;
  const hipError_t e = amph::launch_acc_b64_seg(tx, party, p->d_woff, p->d_foff, K, amph::wire_tile_grid(T, K),
                                                p->sums, p->d_bad, m.dverd, c->f, cfg(c, m.s, T));
  if (e == hipSuccess) p->have |= 1u << party;  // the sums hold this party from here on, whatever its verdict
  if (int st = m.finish(e, "k_acc_b64")) return st;
  const unsigned long long* got = m.verdict_words();
  std::vector<unsigned long long> v(K, amph::kNoFail);  // (no MAC verdicts in a party call)
  v.insert(v.end(), got, got + K);
  for (size_t o = 0; o < K; ++o)
    if (got[o] < p->bad_host[o]) p->bad_host[o] = got[o];
  std::vector<int64_t> none(K), bad(K);
  const int st = wire_batch_status(v.data(), K, p->woff.data(), none.data(), bad.data());
  if (bad_chars) std::copy(bad.begin(), bad.end(), bad_chars);
  return st;
}

int amph_clients_party_dev(amph_clients* p, int party, const amph_odo_b64* texts, int64_t* bad_chars, void* stream) {
  if (int st = clients_check(p, true, true)) return st;
  if (int st = verdicts_misaligned({bad_chars})) return st;
  amph_ctx* c = p->c;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(use_device(c->device));
  std::lock_guard<std::mutex> g(c->mu);
  if (int st = clients_slot_check(p, party, texts)) return st;
  amph::TextSet tx{};
  for (int k = 0; k < 5; ++k) {
    tx.t[k][0] = b64_field(*texts, k);
    if (int st = check_dev_words({tx.t[k][0]})) return st;
  }
  p->dstream = s;
  if (bad_chars) HIP_TRY(hipMemsetAsync(bad_chars, 0x7F, 8 * p->K, s));
  if (p->T) {
    const hipError_t e =
        amph::launch_acc_b64_seg(tx, party, p->d_woff, p->d_foff, p->K, amph::wire_tile_grid(p->T, p->K), p->sums,
                                 p->d_bad, (unsigned long long*)bad_chars, c->f, cfg(c, s, p->T));
    if (e != hipSuccess) return hip_fail(e, "k_acc_b64");
  }
  p->have |= 1u << party;
  return AMPH_OK;
}

int amph_clients_finish_verify(amph_clients* p, uint8_t* out_secrets, int64_t* first_fails, int64_t* bad_chars) {
  return clients_finish_host(p, out_secrets, nullptr, nullptr, nullptr, nullptr, 0, false, false, first_fails,
                             bad_chars);
}

int amph_clients_finish_mask(amph_clients* p, const uint8_t* secrets, uint8_t* out_masked16, char* out_records24,
                             int64_t* first_fails, int64_t* bad_chars) {
  return clients_finish_host(p, nullptr, secrets, out_masked16, out_records24, nullptr, 0, true, false, first_fails,
                             bad_chars);
}

int amph_clients_finish_mask_json(amph_clients* p, const uint8_t* secrets, char* out_text, size_t out_cap,
                                  int64_t* first_fails, int64_t* bad_chars) {
  return clients_finish_host(p, nullptr, secrets, nullptr, nullptr, out_text, out_cap, true, true, first_fails,
                             bad_chars);
}

int amph_clients_finish_verify_dev(amph_clients* p, uint8_t* out_secrets, int64_t* first_fails, int64_t* bad_chars,
                                   void* stream) {
  return clients_finish_dev(p, out_secrets, nullptr, nullptr, nullptr, nullptr, 0, false, false, first_fails,
                            bad_chars, (hipStream_t)stream);
}

int amph_clients_finish_mask_dev(amph_clients* p, const uint8_t* secrets, uint8_t* out_masked16, char* out_records24,
                                 int64_t* first_fails, int64_t* bad_chars, void* stream) {
  return clients_finish_dev(p, nullptr, secrets, out_masked16, out_records24, nullptr, 0, true, false, first_fails,
                            bad_chars, (hipStream_t)stream);
}

int amph_clients_finish_mask_json_dev(amph_clients* p, const uint8_t* secrets, char* out_text, size_t out_cap,
                                      int64_t* first_fails, int64_t* bad_chars, void* stream) {
  return clients_finish_dev(p, nullptr, secrets, nullptr, nullptr, out_text, out_cap, true, true, first_fails,
                            bad_chars, (hipStream_t)stream);
}

int amph_clients_word(amph_clients* p, size_t object, size_t index, uint8_t out_yrvwu[5][16]) {
  if (!p || !p->c) return fail(AMPH_E_PARAM, "null client batch session");
  if (!out_yrvwu) return fail(AMPH_E_PARAM, "null output");
  amph_ctx* c = p->c;
  HIP_TRY(use_device(c->device));
  std::lock_guard<std::mutex> g(c->mu);
  if (int st = clients_all_in(p)) return st;
  if (object >= p->K) return fail(AMPH_E_RANGE, "object " + std::to_string(object) + " of " + std::to_string(p->K));
  const size_t W = (size_t)(p->woff[object + 1] - p->woff[object]);
  if (index >= W)
    return fail(AMPH_E_RANGE, "word " + std::to_string(index) + " of object " + std::to_string(object) + "'s " +
                                  std::to_string(W));
  HIP_TRY(hipStreamSynchronize(p->dstream));
  for (int k = 0; k < 5; ++k) {
    uint4 x;
    HIP_TRY(hipMemcpy(&x, p->sums.s[k] + p->woff[object] + index, 16, hipMemcpyDeviceToHost));  // kPageableRule
    const W4 y = amph::redc(amph::w4(x), c->f);
    std::memcpy(out_yrvwu[k], y.v, 16);
  }
  return AMPH_OK;
}

size_t amph_clients_objects(const amph_clients* p) { return p ? p->K : 0; }
size_t amph_clients_words(const amph_clients* p) { return p ? p->T : 0; }
int amph_clients_parties_seen(const amph_clients* p) { return p ? __builtin_popcount(p->have) : 0; }
size_t amph_clients_field_chars(const amph_clients* p) { return p ? p->field_chars : 0; }
size_t amph_clients_upload_chars(const amph_clients* p) { return p ? p->upload_chars : 0; }

int amph_clients_field_offsets(const amph_clients* p, uint64_t* out) {
  if (!p || !out) return fail(AMPH_E_PARAM, "null client batch session or output");
  std::copy(p->foff.begin(), p->foff.end(), out);
  return AMPH_OK;
}

int amph_clients_upload_offsets(const amph_clients* p, uint64_t* out) {
  if (!p || !out) return fail(AMPH_E_PARAM, "null client batch session or output");
  std::copy(p->uoff.begin(), p->uoff.end(), out);
  return AMPH_OK;
}

uint64_t amph_clients_copies(const amph_ctx* c) {
  return c ? first_device(c)->clients_copies.load(std::memory_order_relaxed) : 0;
}

void amph_clients_free(amph_clients* p) {
  if (!p) return;
  if (p->c) {
    (void)use_device(p->c->device);
    std::lock_guard<std::mutex> g(p->c->mu);
    if (p->dstream) (void)hipStreamSynchronize(p->dstream);
    pool_put(p->c, p->mem);  // back to the context for the next session
  }
  delete p;
}

}  // extern "C"
