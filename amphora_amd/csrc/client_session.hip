// C ABI of libamphora_hip (declared in include/amphora_client_session.h): the
// client side as a session -- each party's five base64 texts are added into
// five running sums on the device as they arrive (k_acc_b64, one launch per
// party), and the finish calls run K_RV / K_MASK from the sums alone.
//
// Device memory: one pooled buffer (the party sessions' pool) carved into the
// five sums and the session's bad-character word.  Host mode stages one
// party's texts, and the finish call's secrets and outputs, through the
// context's Stager exactly as the whole wire-text calls do: the small-call
// arena, or the context's wire staging buffer with blocking copies while the
// context's stream is idle (kPageableRule).  Every launch of a host session
// goes on the context's first stream under the context's mutex, every launch
// of a device session on the caller's stream, so the read-modify-write on the
// sums runs in order.
#include "capi_internal.hpp"

struct amph_client {
  amph_ctx* c = nullptr;
  size_t W = 0, nchars = 0;
  uint32_t pad = 0;
  int n = 0;
  bool dev = false;
  hipStream_t dstream = nullptr;  // device mode: the stream of the latest call
  DevBuf mem;
  amph::SumSet sums{};
  unsigned long long* bad = nullptr;  // min over the parties, whole-call encoding (device word)
  int64_t bad_host = (int64_t)AMPH_NO_FAILURE;  // host mode: the same, as the party calls returned it
  uint32_t have = 0;  // bit j: party j's texts are in the sums
  bool finished = false;
};

namespace {
int client_check(amph_client* p, bool dev, bool open) {
  if (!p || !p->c) return fail(AMPH_E_PARAM, "null client session");
  if (p->dev != dev)
    return fail(AMPH_E_PARAM, dev ? "a host-mode client session takes the host calls"
                                  : "a device-mode client session takes the *_dev calls");
  if (open && p->finished) return fail(AMPH_E_PARAM, "the client session is already finished");
  return AMPH_OK;
}

int client_missing(const amph_client* p) {  // the first open slot, -1: all in
  for (int j = 0; j < p->n; ++j)
    if (!(p->have >> j & 1u)) return j;
  return -1;
}

int client_all_in(const amph_client* p) {
  const int j = client_missing(p);
  if (j < 0) return AMPH_OK;
  return fail(AMPH_E_PARAM, "party " + std::to_string(j) + "'s texts are missing");
}

int client_begin(amph_ctx* c, size_t words, int n_parties, bool dev, hipStream_t stream, amph_client** out) {
  if (!out) return fail(AMPH_E_PARAM, "null session output");
  *out = nullptr;
  if (check_ctx(c)) return AMPH_E_PARAM;
  if (n_parties < 1 || n_parties > AMPH_MAX_PARTIES) return fail(AMPH_E_PARAM, "n_parties must be in [1, 16]");
  if (dev && !c->sub.empty()) return fail(AMPH_E_PARAM, "device-mode sessions need a single-device context");
  c = first_device(c);  // a multi-device context runs sessions on its first device
  HIP_TRY(use_device(c->device));
  std::lock_guard<std::mutex> g(c->mu);
  std::unique_ptr<amph_client> p(new amph_client);
  p->c = c;
  p->W = words;
  p->n = n_parties;
  p->dev = dev;
  p->nchars = b64_chars(16 * words);
  p->pad = (uint32_t)((3 - (16 * words) % 3) % 3);
  if (dev) p->dstream = stream;
  else if (int st = host_stream(c, 0, &p->dstream)) return st;
  if (words) {
    const size_t field = align256(16 * words);
    if (pool_ensure(c, p->mem, 5 * field + 256) != hipSuccess)
      return fail(AMPH_E_NOMEM, "client session device memory");
    uint8_t* base = (uint8_t*)p->mem.p;
    for (int k = 0; k < 5; ++k) p->sums.s[k] = (uint4*)(base + k * field);
    p->bad = (unsigned long long*)(base + 5 * field);
    hipError_t e = hipMemsetAsync(base, 0, 5 * field, p->dstream);
    if (e == hipSuccess) e = hipMemsetAsync(p->bad, 0x7F, 8, p->dstream);
    // host mode: the context's stream is idle between host calls (kPageableRule)
    if (e == hipSuccess && !dev) e = hipStreamSynchronize(p->dstream);
    if (e != hipSuccess) {
      pool_put(c, p->mem);
      return hip_fail(e, "client session sums");
    }
  }
  *out = p.release();
  return AMPH_OK;
}

// what every party call checks before anything is launched (c->mu held)
int client_slot_check(amph_client* p, int party, const amph_odo_b64* texts) {
  if (!texts) return fail(AMPH_E_PARAM, "null texts");
  if (party < 0 || party >= p->n)
    return fail(AMPH_E_PARAM, "party must be in [0, " + std::to_string(p->n - 1) + "]");
  if (p->have >> party & 1u) return fail(AMPH_E_PARAM, "party " + std::to_string(party) + "'s slot is already taken");
  if (texts->nchars != p->nchars)
    return fail(AMPH_E_LEN, "party " + std::to_string(party) + ": base64 fields of " + std::to_string(texts->nchars) +
                                " characters, expected " + std::to_string(p->nchars) + " for " +
                                std::to_string(p->W) + " words");
  for (int k = 0; k < 5 && p->W; ++k)
    if (!b64_field(*texts, k)) return fail(AMPH_E_PARAM, "null ODO field text");
  return AMPH_OK;
}

amph::OdoSet client_odo(const amph_client* p) {  // the sums as a one-party ODO of canonical words
  amph::OdoSet o{};
  for (int k = 0; k < 5; ++k) o.f[k][0] = p->sums.s[k];
  return o;
}

// the MAC verdict of a host-mode finish (a bad character was reported before the launch)
int client_status(int64_t ff, int64_t* first_fail) {
  if (ff != (int64_t)AMPH_NO_FAILURE) {
    if (first_fail) *first_fail = ff;
    return AMPH_E_VERIFY;
  }
  return AMPH_OK;
}

// Host mode of the finish calls: verify (out_y) or mask (the other outputs).
int client_finish_host(amph_client* p, uint8_t* out_y, const uint8_t* secrets, size_t n_secrets, uint8_t* out16,
                       char* out24, char* out_text, size_t out_cap, bool mask, bool json, int64_t* first_fail,
                       int64_t* bad_char) {
  if (int st = client_check(p, false, true)) return st;
  amph_ctx* c = p->c;
  const size_t W = p->W;
  if (mask && json && !out_text && n_secrets <= W) return fail(AMPH_E_PARAM, "null output text");
  if (!mask && W && !out_y) return fail(AMPH_E_PARAM, "null output");
  HIP_TRY(use_device(c->device));
  std::lock_guard<std::mutex> g(c->mu);
  if (int st = client_all_in(p)) return st;
  if (first_fail) *first_fail = -1;
  if (bad_char) *bad_char = -1;
  if (p->bad_host != (int64_t)AMPH_NO_FAILURE) {  // known from the party calls: nothing to launch
    p->finished = true;
    if (bad_char) *bad_char = p->bad_host;
    return wire_bad_message(p->bad_host, p->nchars);
  }
  const bool over = mask && n_secrets > W;  // every mask verifies before the length error
  if (!over) {
    if (mask && n_secrets && !secrets) return fail(AMPH_E_PARAM, "null secrets");
    if (out_text && out_cap < amph_masked_input_data_chars(n_secrets))
      return fail(AMPH_E_LEN, "output capacity " + std::to_string(out_cap) + " below the " +
                                  std::to_string(amph_masked_input_data_chars(n_secrets)) + " characters of " +
                                  std::to_string(n_secrets) + " records");
  }
  p->finished = true;
  const size_t S = over ? 0 : n_secrets;
  const size_t text_chars = amph_masked_input_data_chars(S);
  char* const empty_text = out_text && S == 0 && !over ? out_text : nullptr;  // "[]", once the masks verified
  if (over || empty_text) out16 = nullptr, out24 = nullptr, out_text = nullptr;
  if (W) {
    hipStream_t s = p->dstream;
    Stager h;
    const size_t bytes = mask ? 3 * align256(16 * S) + align256(24 * S) + (out_text ? align256(text_chars) : 0) + 1024
                              : align256(16 * W) + 512;
    const bool small = small_call(c, bytes);
    if (int st = h.begin(c, s, small, bytes, 1, &c->wire, small ? 0 : bytes, "wire staging")) return st;
    hipError_t e;
    int64_t v = 0;
    if (!mask) {
      uint8_t* dout = h.take(16 * W);
      if (int st = h.arm()) return st;
      e = amph::launch_recombine_verify(client_odo(p), 1, W, (uint4*)dout, h.fl, c->f, cfg(c, s, W));
      if (e != hipSuccess) return h.launch_failed(e, "k_rv");
      if (int st = h.finish(&v, {})) return st;
      if (int st = client_status(v, first_fail)) return st;
      return h.fetch({{out_y, dout, 16 * W}});
    }
    uint8_t* dsec = h.take(16 * S);
    uint8_t* d16 = h.take(16 * S);
    uint8_t* d24 = h.take(24 * S);
    uint8_t* dtext = out_text ? h.take(text_chars) : nullptr;
    if (S) HIP_TRY(h.put(dsec, secrets, 16 * S));
    if (int st = h.arm()) return st;
    e = amph::launch_mask_sums(p->sums, W, (const uint4*)dsec, S, out16 ? (uint4*)d16 : nullptr,
                               out24 ? (char*)d24 : nullptr, (char*)dtext, h.fl, c->f, cfg(c, s, W));
    if (e != hipSuccess) return h.launch_failed(e, "k_mask_sums");
    if (int st = h.finish(&v, {})) return st;
    if (int st = client_status(v, first_fail)) return st;
    if (int st = h.fetch({{out16, d16, out16 ? 16 * S : 0},
                          {out24, d24, out24 ? 24 * S : 0},
                          {out_text, dtext, out_text ? text_chars : 0}}))
      return st;
  }
  if (over) return fail(AMPH_E_LEN, "more secret words than verified input masks");
  if (empty_text) empty_text[0] = '[', empty_text[1] = ']';
  return AMPH_OK;
}

// Device mode of the finish calls.
int client_finish_dev(amph_client* p, uint8_t* out_y, const uint8_t* secrets, size_t n_secrets, uint8_t* out16,
                      char* out24, char* out_text, size_t out_cap, bool mask, bool json, int64_t* first_fail,
                      int64_t* bad_char, hipStream_t s) {
  if (int st = client_check(p, true, true)) return st;
  amph_ctx* c = p->c;
  const size_t W = p->W;
  if (mask && json && !out_text && n_secrets <= W) return fail(AMPH_E_PARAM, "null output text");
  if (!mask && W && !out_y) return fail(AMPH_E_PARAM, "null output");
  if (int st = check_dev_words({out_y, secrets, out16, out24, out_text})) return st;
  HIP_TRY(use_device(c->device));
  std::lock_guard<std::mutex> g(c->mu);
  if (int st = client_all_in(p)) return st;
  const bool over = mask && n_secrets > W;
  if (!over) {
    if (mask && n_secrets && !secrets) return fail(AMPH_E_PARAM, "null secrets");
    if (out_text && out_cap < amph_masked_input_data_chars(n_secrets))
      return fail(AMPH_E_LEN, "output capacity " + std::to_string(out_cap) + " below the " +
                                  std::to_string(amph_masked_input_data_chars(n_secrets)) + " characters of " +
                                  std::to_string(n_secrets) + " records");
  }
  if (int st = reset_ff_dev(first_fail, 0, s)) return st;
  if (int st = reset_ff_dev(bad_char, 0, s)) return st;
  p->dstream = s;
  p->finished = true;
  const size_t S = over ? 0 : n_secrets;
  if (over) out16 = nullptr, out24 = nullptr, out_text = nullptr;
  if (out_text && S == 0) {  // no secrets: "[]", and the masks are still verified
    HIP_TRY(hipMemsetAsync(out_text, '[', 1, s));
    HIP_TRY(hipMemsetAsync(out_text + 1, ']', 1, s));
    out_text = nullptr;
  }
  if (W) {
    HIP_TRY(hipMemcpyAsync(bad_char, p->bad, 8, hipMemcpyDeviceToDevice, s));
    hipError_t e = mask ? amph::launch_mask_sums(p->sums, W, (const uint4*)secrets, S, (uint4*)out16, out24, out_text,
                                                 (unsigned long long*)first_fail, c->f, cfg(c, s, W))
                        : amph::launch_recombine_verify(client_odo(p), 1, W, (uint4*)out_y,
                                                        (unsigned long long*)first_fail, c->f, cfg(c, s, W));
    if (e != hipSuccess) return hip_fail(e, mask ? "k_mask_sums" : "k_rv");
  }
  if (!over) return AMPH_OK;
  // as the whole call: the verdicts are read before the length error is reported
  HIP_TRY(hipStreamSynchronize(s));
  int64_t v[2];
  HIP_TRY(hipMemcpy(&v[0], first_fail, 8, hipMemcpyDeviceToHost));  // kPageableRule
  HIP_TRY(hipMemcpy(&v[1], bad_char, 8, hipMemcpyDeviceToHost));
  if (v[1] != (int64_t)AMPH_NO_FAILURE) return wire_bad_message(v[1], p->nchars);
  if (v[0] != (int64_t)AMPH_NO_FAILURE)
    return fail(AMPH_E_VERIFY, "input mask MAC check failed at word " + std::to_string(v[0]));
  return fail(AMPH_E_LEN, "more secret words than verified input masks");
}
}  // namespace

extern "C" {

int amph_client_begin(amph_ctx* c, size_t words, int n_parties, amph_client** out) {
  return client_begin(c, words, n_parties, false, nullptr, out);
}

int amph_client_begin_dev(amph_ctx* c, size_t words, int n_parties, void* stream, amph_client** out) {
  return client_begin(c, words, n_parties, true, (hipStream_t)stream, out);
}

int amph_client_party(amph_client* p, int party, const amph_odo_b64* texts, int64_t* bad_char) {
  if (bad_char) *bad_char = -1;
  if (int st = client_check(p, false, true)) return st;
  amph_ctx* c = p->c;
  HIP_TRY(use_device(c->device));
  std::lock_guard<std::mutex> g(c->mu);
  if (int st = client_slot_check(p, party, texts)) return st;
  if (p->W == 0) {
    p->have |= 1u << party;
    return AMPH_OK;
  }
  hipStream_t s = p->dstream;
  Stager h;
  const size_t bytes = 5 * align256(p->nchars) + 256;
  const bool small = small_call(c, bytes);
  if (int st = h.begin(c, s, small, bytes, 1, &c->wire, small ? 0 : bytes, "wire staging")) return st;
  amph::TextSet tx{};
  for (int k = 0; k < 5; ++k) {
    uint8_t* d = h.take(p->nchars);
    HIP_TRY(h.put(d, b64_field(*texts, k), p->nchars));
    tx.t[k][0] = (const char*)d;
  }
  if (int st = h.arm()) return st;
  hipError_t e = amph::launch_acc_b64(tx, party, p->W, p->nchars, p->pad, p->sums, p->bad, h.fl, c->f,
                                      cfg(c, s, p->W));
  if (e != hipSuccess) return h.launch_failed(e, "k_acc_b64");
  p->have |= 1u << party;  // the sums hold this party from here on, whatever its verdict
  int64_t v = 0;
  if (int st = h.finish(&v, {})) return st;
  if (v == (int64_t)AMPH_NO_FAILURE) return AMPH_OK;
  if (p->bad_host == (int64_t)AMPH_NO_FAILURE || v < p->bad_host) p->bad_host = v;
  if (bad_char) *bad_char = v;
  return wire_bad_message(v, p->nchars);
}

int amph_client_party_dev(amph_client* p, int party, const amph_odo_b64* texts, int64_t* bad_char, void* stream) {
  if (int st = client_check(p, true, true)) return st;
  amph_ctx* c = p->c;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(use_device(c->device));
  std::lock_guard<std::mutex> g(c->mu);
  if (int st = client_slot_check(p, party, texts)) return st;
  amph::TextSet tx{};
  for (int k = 0; k < 5; ++k) {
    tx.t[k][0] = b64_field(*texts, k);
    if (int st = check_dev_words({tx.t[k][0]})) return st;
  }
  if (int st = reset_ff_dev(bad_char, 0, s)) return st;
  p->dstream = s;
  hipError_t e = amph::launch_acc_b64(tx, party, p->W, p->nchars, p->pad, p->sums, p->bad,
                                      (unsigned long long*)bad_char, c->f, cfg(c, s, p->W));
  if (e != hipSuccess) return hip_fail(e, "k_acc_b64");
  p->have |= 1u << party;
  return AMPH_OK;
}

int amph_client_finish_verify(amph_client* p, uint8_t* out_secrets, int64_t* first_fail, int64_t* bad_char) {
  return client_finish_host(p, out_secrets, nullptr, 0, nullptr, nullptr, nullptr, 0, false, false, first_fail,
                            bad_char);
}

int amph_client_finish_mask(amph_client* p, const uint8_t* secrets, size_t n_secrets, uint8_t* out_masked16,
                            char* out_records24, int64_t* first_fail, int64_t* bad_char) {
  return client_finish_host(p, nullptr, secrets, n_secrets, out_masked16, out_records24, nullptr, 0, true, false,
                            first_fail, bad_char);
}

int amph_client_finish_mask_json(amph_client* p, const uint8_t* secrets, size_t n_secrets, char* out_text,
                                 size_t out_cap, int64_t* first_fail, int64_t* bad_char) {
  return client_finish_host(p, nullptr, secrets, n_secrets, nullptr, nullptr, out_text, out_cap, true, true,
                            first_fail, bad_char);
}

int amph_client_finish_verify_dev(amph_client* p, uint8_t* out_secrets, int64_t* first_fail, int64_t* bad_char,
                                  void* stream) {
  return client_finish_dev(p, out_secrets, nullptr, 0, nullptr, nullptr, nullptr, 0, false, false, first_fail,
                           bad_char, (hipStream_t)stream);
}

int amph_client_finish_mask_dev(amph_client* p, const uint8_t* secrets, size_t n_secrets, uint8_t* out_masked16,
                                char* out_records24, int64_t* first_fail, int64_t* bad_char, void* stream) {
  return client_finish_dev(p, nullptr, secrets, n_secrets, out_masked16, out_records24, nullptr, 0, true, false,
                           first_fail, bad_char, (hipStream_t)stream);
}

int amph_client_finish_mask_json_dev(amph_client* p, const uint8_t* secrets, size_t n_secrets, char* out_text,
                                     size_t out_cap, int64_t* first_fail, int64_t* bad_char, void* stream) {
  return client_finish_dev(p, nullptr, secrets, n_secrets, nullptr, nullptr, out_text, out_cap, true, true,
                           first_fail, bad_char, (hipStream_t)stream);
}

int amph_client_word(amph_client* p, size_t index, uint8_t out_yrvwu[5][16]) {
  if (!p || !p->c) return fail(AMPH_E_PARAM, "null client session");
  if (!out_yrvwu) return fail(AMPH_E_PARAM, "null output");
  amph_ctx* c = p->c;
  HIP_TRY(use_device(c->device));
  std::lock_guard<std::mutex> g(c->mu);
  if (int st = client_all_in(p)) return st;
  if (index >= p->W)
    return fail(AMPH_E_RANGE, "word " + std::to_string(index) + " of a session of " + std::to_string(p->W));
  HIP_TRY(hipStreamSynchronize(p->dstream));
  for (int k = 0; k < 5; ++k) {
    uint4 x;
    HIP_TRY(hipMemcpy(&x, p->sums.s[k] + index, 16, hipMemcpyDeviceToHost));  // kPageableRule
    const W4 y = amph::redc(amph::w4(x), c->f);
    std::memcpy(out_yrvwu[k], y.v, 16);
  }
  return AMPH_OK;
}

size_t amph_client_words(const amph_client* p) { return p ? p->W : 0; }

int amph_client_parties_seen(const amph_client* p) { return p ? __builtin_popcount(p->have) : 0; }

void amph_client_free(amph_client* p) {
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
