// C ABI of libamphora_hip (declared in include/amphora.h): one party's Output
// Delivery as a session, and the context's pool of session buffers.
#include "capi_internal.hpp"

// ---- one party's Output Delivery, device-resident between steps ----------------
// (include/amphora.h, "one party's Output Delivery with device-resident state")
// Device memory: one allocation carved into the triples (host mode), the five
// ODO fields, this party's diffs, its text and the encoder's scratch; the share
// data and masks live in a second one released once begin has run; each
// partner's diffs (the exchange decode's span form, amph::XSpans) and its
// decode scratch in one allocation per slot, sized by its text; partner texts
// and the base64 output staged in a fourth (host mode).  Host mode: every copy
// is a blocking hipMemcpy issued with the context's stream idle
// (kPageableRule), so caller buffers may be pageable or page-locked.  Device
// mode (amph_party_*_dev): nothing is copied; the caller's buffers are used in
// place and every launch goes on the caller's stream.
struct amph_party {
  amph_ctx* c = nullptr;
  size_t W = 0;
  int n = 0;
  bool dev = false;               // device mode
  hipStream_t dstream = nullptr;  // device mode: the stream of the latest call
  DevBuf mem, tmp, io;
  const uint4* triples = nullptr;
  uint4* f5[5] = {};  // y, r, v, w, u
  char* b64[5] = {};  // the five fields as base64 text (finish_b64)
  uint4* mag[AMPH_MAX_PARTIES] = {};
  uint8_t* neg[AMPH_MAX_PARTIES] = {};
  DevBuf pbuf[AMPH_MAX_PARTIES];
  amph::XSpans xs[AMPH_MAX_PARTIES] = {};
  char* text = nullptr;
  unsigned long long* text_len_dev = nullptr;
  void* enc_scratch = nullptr;
  uint64_t* enc_lens = nullptr;  // K_ODO_PRE's exchange text lengths, scanned by the encode
  uint64_t text_len = 0;
  uint32_t have = 0;  // bit j: party j's diffs are on the device (bit 0 after begin)
  const unsigned long long* bad_dev[AMPH_MAX_PARTIES] = {};  // device mode: partner verdict words
  // device mode: the session's own copies of the partner verdicts, and per
  // slot an event after the partner call's work (finish may use another stream)
  DevBuf verdicts;
  hipEvent_t partner_ev[AMPH_MAX_PARTIES] = {};
  bool finished = false;
  ~amph_party() {
    mem.release();
    tmp.release();
    io.release();
    verdicts.release();
    for (DevBuf& b : pbuf) b.release();
    for (hipEvent_t& e : partner_ev)
      if (e) (void)hipEventDestroy(e);
  }
};

namespace capi __attribute__((visibility("hidden"))) {
// (declared in capi_internal.hpp: parties_session.hip shares them)
void pool_put(amph_ctx* c, DevBuf& b) {
  if (!b.p) return;
  c->party_pool.push_back(b);
  b.p = nullptr;
  b.cap = 0;
  while (!c->party_pool.empty() &&
         (c->party_pool.size() > kPartyPoolMax || pool_bytes(c) > c->pool_cap_bytes)) {
    size_t m = 0;
    for (size_t i = 1; i < c->party_pool.size(); ++i)
      if (c->party_pool[i].cap < c->party_pool[m].cap) m = i;
    c->party_pool[m].release();
    c->party_pool.erase(c->party_pool.begin() + (long)m);
  }
}

hipError_t pool_ensure(amph_ctx* c, DevBuf& b, size_t bytes) {
  if (bytes <= b.cap) return hipSuccess;
  pool_put(c, b);
  long best = -1;
  for (size_t i = 0; i < c->party_pool.size(); ++i)
    if (c->party_pool[i].cap >= bytes && (best < 0 || c->party_pool[i].cap < c->party_pool[(size_t)best].cap))
      best = (long)i;
  if (best >= 0) {
    b = c->party_pool[(size_t)best];
    c->party_pool.erase(c->party_pool.begin() + best);
    return hipSuccess;
  }
  return dev_ensure(c, b, bytes);
}
}  // namespace capi

namespace {
int party_check(amph_party* p) {
  if (!p || !p->c) return fail(AMPH_E_PARAM, "null party session");
  if (p->finished) return fail(AMPH_E_PARAM, "the party session is already finished");
  return AMPH_OK;
}

int party_args(amph_ctx* c, size_t share_stride, int n_parties, size_t words, const void* share_data,
               const void* masks, const void* triples, amph_party** out) {
  if (!out) return fail(AMPH_E_PARAM, "null session output");
  *out = nullptr;
  if (check_ctx(c)) return AMPH_E_PARAM;
  if (share_stride != 16 && share_stride != 32) return fail(AMPH_E_PARAM, "share_stride must be 16 or 32");
  if (n_parties < 1 || n_parties > AMPH_MAX_PARTIES) return fail(AMPH_E_PARAM, "n_parties must be in [1, 16]");
  if (words && (!share_data || !masks || !triples)) return fail(AMPH_E_PARAM, "null buffer");
  return AMPH_OK;
}

// the session's device memory; yrv[k] non-null: field k lives in the caller's
// device buffer (device mode), else in the session's
int party_alloc(amph_party* p, bool copy_triples, uint8_t* const yrv[3]) {
  const size_t W = p->W, P = 2 * W, nc = b64_chars(16 * W);
  const size_t nl = (P + amph::kXLenPairs - 1) / amph::kXLenPairs;
  const size_t sz[] = {copy_triples ? 192 * W : 0, 16 * W, 16 * W, 16 * W, 16 * W, 16 * W,
                       amph::xenc_max_bytes(P), 8, amph::xenc_lens_scratch_bytes(P), 64 * W, 4 * W, nc, nc, nc, nc, nc,
                       8 * (nl + 1)};
  size_t total = 0;
  for (size_t b : sz) total += align256(b ? b : 16);
  if (pool_ensure(p->c, p->mem, total) != hipSuccess) return fail(AMPH_E_NOMEM, "party session device memory");
  uint8_t* cur = (uint8_t*)p->mem.p;
  auto take = [&](size_t b) {
    uint8_t* q = cur;
    cur += align256(b ? b : 16);
    return q;
  };
  p->triples = (const uint4*)take(sz[0]);
  for (int k = 0; k < 5; ++k) {
    uint4* own = (uint4*)take(sz[1 + k]);
    p->f5[k] = k < 3 && yrv[k] ? (uint4*)yrv[k] : own;
  }
  p->text = (char*)take(sz[6]);
  p->text_len_dev = (unsigned long long*)take(sz[7]);
  p->enc_scratch = take(sz[8]);
  p->mag[0] = (uint4*)take(sz[9]);
  p->neg[0] = take(sz[10]);
  for (int k = 0; k < 5; ++k) p->b64[k] = (char*)take(sz[11 + k]);
  p->enc_lens = (uint64_t*)take(sz[16]);
  return AMPH_OK;
}

// k_odo_pre (y, r, v + this party's diffs and their exchange text lengths)
// and the exchange encode of the diffs
int party_pre(amph_party* p, const uint8_t* dshare, size_t share_stride, const uint8_t* dmasks, hipStream_t s) {
  amph_ctx* c = p->c;
  const size_t W = p->W, P = 2 * W;
  hipError_t e = amph::launch_odo_pre((const uint4*)dshare, (int)(share_stride / 16), (const uint4*)dmasks,
                                      p->triples, W, p->f5[0], p->f5[1], p->f5[2], p->mag[0], (uint32_t*)p->neg[0],
                                      c->f, cfg(c, s, W), p->enc_lens);
  if (e != hipSuccess) return hip_fail(e, "k_odo_pre");
  e = amph::launch_exchange_encode_lens(p->mag[0], p->neg[0], P, p->enc_lens, p->text, p->text_len_dev,
                                        p->enc_scratch, cfg(c, s, P));
  return e == hipSuccess ? AMPH_OK : hip_fail(e, "k_xenc");
}

int party_slot_check(amph_party* p, int slot, const char* text, size_t len) {
  if (int st = party_check(p)) return st;
  if (slot < 1 || slot >= p->n)
    return fail(AMPH_E_PARAM, "partner slot must be in [1, " + std::to_string(p->n - 1) + "]");
  if (p->have >> slot & 1u) return fail(AMPH_E_PARAM, "partner slot " + std::to_string(slot) + " already holds a text");
  if (len && !text) return fail(AMPH_E_PARAM, "null text");
  return AMPH_OK;
}

// a partner's text (device memory) decoded into the slot's span form; bad:
// the device word the decode reports into (reset by its first kernel)
int party_decode(amph_party* p, int slot, const char* dtext, size_t len, unsigned long long* bad, hipStream_t s) {
  const size_t P = 2 * p->W;
  const size_t nb = amph::xspan_spans(len), slots = amph::xspan_slots(len, P);
  const size_t xsz[5] = {16 * slots, slots, 8 * (nb + 1), 16 * amph::xspan_map_words(P),
                         amph::xdec_spans_scratch_bytes(len)};
  size_t xtotal = 0;
  for (size_t b : xsz) xtotal += align256(b);
  if (pool_ensure(p->c, p->pbuf[slot], xtotal) != hipSuccess)
    return fail(AMPH_E_NOMEM, "party session partner diffs");
  uint8_t* xp = (uint8_t*)p->pbuf[slot].p;
  amph::XSpans& xs = p->xs[slot];
  xs.mag = (uint4*)xp;
  xs.neg = xp + align256(xsz[0]);
  xs.base = (uint64_t*)(xs.neg + align256(xsz[1]));
  xs.map = (uint4*)((uint8_t*)xs.base + align256(xsz[2]));
  void* scratch = (uint8_t*)xs.map + align256(xsz[3]);
  xs.nb = nb;
  p->mag[slot] = xs.mag;
  p->neg[slot] = xs.neg;
  hipError_t e = amph::launch_exchange_decode_spans(dtext, len, P, xs, bad, scratch, cfg(p->c, s, len));
  return e == hipSuccess ? AMPH_OK : hip_fail(e, "k_xdec");
}

int party_all_in(amph_party* p) {
  const uint32_t all = p->n >= 32 ? ~0u : ((1u << p->n) - 1u);
  if ((p->have & all) == all) return AMPH_OK;
  int j = 1;
  while (j < p->n && (p->have >> j & 1u)) ++j;
  return fail(AMPH_E_PARAM, "partner slot " + std::to_string(j) + "'s interimValues text is missing");
}

// the summed diffs -> w, u on the device (every partner's text must be in)
int party_open_post(amph_party* p, int is_player0, hipStream_t s) {
  if (int st = party_all_in(p)) return st;
  amph::SignedSet set{};
  for (int j = 0; j < p->n; ++j) {
    set.mag[j] = p->mag[j];
    set.neg[j] = (const uint32_t*)p->neg[j];
    if (j > 0) {
      set.sbase[j] = p->xs[j].base;
      set.smap[j] = p->xs[j].map;
      set.snb[j] = p->xs[j].nb;
    }
  }
  hipError_t e = amph::launch_open_post(set, p->n, p->triples, p->W, is_player0, p->f5[3], p->f5[4], p->c->f,
                                        cfg(p->c, s, p->W));
  return e == hipSuccess ? AMPH_OK : hip_fail(e, "k_open_post");
}

// the five fields as base64 text in the session's memory (one launch)
int party_b64(amph_party* p, hipStream_t s) {
  const size_t nb = 16 * p->W;
  const uint8_t* const in[5] = {(const uint8_t*)p->f5[0], (const uint8_t*)p->f5[1], (const uint8_t*)p->f5[2],
                                (const uint8_t*)p->f5[3], (const uint8_t*)p->f5[4]};
  hipError_t e = amph::launch_b64_encode_multi(in, p->b64, 5, nb, cfg(p->c, s, (nb + 11) / 12));
  return e == hipSuccess ? AMPH_OK : hip_fail(e, "k_b64_encode_multi");
}

int party_mode(amph_party* p, bool dev) {
  if (p->dev != dev)
    return fail(AMPH_E_PARAM, dev ? "a host-mode party session takes the host calls"
                                  : "a device-mode party session takes the *_dev calls");
  return AMPH_OK;
}
}  // namespace

extern "C" {

int amph_party_begin(amph_ctx* c, const uint8_t* share_data, size_t share_stride, const uint8_t* masks,
                     const uint8_t* triples, size_t words, int n_parties, uint8_t* oy, uint8_t* orr,
                     uint8_t* ov, amph_party** out) {
  if (int st = party_args(c, share_stride, n_parties, words, share_data, masks, triples, out)) return st;
  c = first_device(c);  // a multi-device context runs sessions on its first device
  HIP_TRY(use_device(c->device));
  std::lock_guard<std::mutex> g(c->mu);
  std::unique_ptr<amph_party> p(new amph_party);
  p->c = c;
  p->W = words;
  p->n = n_parties;
  const size_t W = words;
  uint8_t* const none[3] = {nullptr, nullptr, nullptr};
  if (int st = party_alloc(p.get(), true, none)) return st;
  if (pool_ensure(c, p->tmp, align256(share_stride * W + 16) + align256(64 * W + 16)) != hipSuccess)
    return fail(AMPH_E_NOMEM, "party session staging");
  uint8_t* dshare = (uint8_t*)p->tmp.p;
  uint8_t* dmasks = dshare + align256(share_stride * W + 16);
  hipStream_t s;
  if (int st = host_stream(c, 0, &s)) return st;
  HIP_TRY(hipStreamSynchronize(s));
  if (W) {
    HIP_TRY(hipMemcpy(dshare, share_data, share_stride * W, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dmasks, masks, 64 * W, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy((void*)p->triples, triples, 192 * W, hipMemcpyHostToDevice));
  }
  if (int st = party_pre(p.get(), dshare, share_stride, dmasks, s)) return st;
  uint64_t len = 0;
  HIP_TRY(read_back(s, {{&len, p->text_len_dev, 8}, {oy, p->f5[0], oy ? 16 * W : 0},
                        {orr, p->f5[1], orr ? 16 * W : 0}, {ov, p->f5[2], ov ? 16 * W : 0}}));
  p->text_len = len;
  p->have = 1u;
  pool_put(c, p->tmp);
  *out = p.release();
  return AMPH_OK;
}

size_t amph_party_words(const amph_party* p) { return p ? p->W : 0; }

uint64_t amph_party_text_len(const amph_party* p) { return p && !p->dev ? p->text_len : 0; }

int amph_party_text(amph_party* p, char* out, size_t out_cap) {
  if (!p || !p->c) return fail(AMPH_E_PARAM, "null party session");
  if (int st = party_mode(p, false)) return st;
  if (!out && p->text_len) return fail(AMPH_E_PARAM, "null output");
  if (out_cap < p->text_len)
    return fail(AMPH_E_LEN, "output capacity " + std::to_string(out_cap) + " below the text length " +
                                std::to_string(p->text_len));
  amph_ctx* c = p->c;
  HIP_TRY(use_device(c->device));
  std::lock_guard<std::mutex> g(c->mu);
  hipStream_t s;
  if (int st = host_stream(c, 0, &s)) return st;
  HIP_TRY(read_back(s, {{out, p->text, p->text_len}}));
  return AMPH_OK;
}

int amph_party_partner(amph_party* p, int slot, const char* text, size_t len, int64_t* bad_index) {
  if (bad_index) *bad_index = -1;
  if (int st = party_slot_check(p, slot, text, len)) return st;
  if (int st = party_mode(p, false)) return st;
  amph_ctx* c = p->c;
  HIP_TRY(use_device(c->device));
  std::lock_guard<std::mutex> g(c->mu);
  if (pool_ensure(c, p->io, align256(len + 16) + 256) != hipSuccess)
    return fail(AMPH_E_NOMEM, "party session text staging");
  uint8_t* dtext = (uint8_t*)p->io.p;
  unsigned long long* dbad = (unsigned long long*)(dtext + align256(len + 16));
  hipStream_t s;
  if (int st = host_stream(c, 0, &s)) return st;
  HIP_TRY(hipStreamSynchronize(s));
  if (len) HIP_TRY(hipMemcpy(dtext, text, len, hipMemcpyHostToDevice));
  if (int st = party_decode(p, slot, (const char*)dtext, len, dbad, s)) return st;
  int64_t bad = 0;
  HIP_TRY(read_back(s, {{&bad, dbad, 8}}));
  if (int st = decode_status(bad, len, 2 * p->W, bad_index)) return st;
  p->have |= 1u << slot;
  return AMPH_OK;
}

int amph_party_finish(amph_party* p, int is_player0, uint8_t* ow, uint8_t* ou) {
  if (int st = party_check(p)) return st;
  if (int st = party_mode(p, false)) return st;
  if (p->W && (!ow || !ou)) return fail(AMPH_E_PARAM, "null output");
  amph_ctx* c = p->c;
  HIP_TRY(use_device(c->device));
  std::lock_guard<std::mutex> g(c->mu);
  hipStream_t s;
  if (int st = host_stream(c, 0, &s)) return st;
  if (int st = party_open_post(p, is_player0, s)) return st;
  HIP_TRY(read_back(s, {{ow, p->f5[3], 16 * p->W}, {ou, p->f5[4], 16 * p->W}}));
  p->finished = true;
  return AMPH_OK;
}

int amph_party_finish_b64(amph_party* p, int is_player0, char* const fields_b64[5]) {
  if (int st = party_check(p)) return st;
  if (int st = party_mode(p, false)) return st;
  if (!fields_b64) return fail(AMPH_E_PARAM, "null field array");
  for (int k = 0; k < 5; ++k)
    if (p->W && !fields_b64[k]) return fail(AMPH_E_PARAM, "null field text");
  amph_ctx* c = p->c;
  HIP_TRY(use_device(c->device));
  std::lock_guard<std::mutex> g(c->mu);
  const size_t nc = b64_chars(16 * p->W);
  hipStream_t s;
  if (int st = host_stream(c, 0, &s)) return st;
  if (int st = party_open_post(p, is_player0, s)) return st;
  if (int st = party_b64(p, s)) return st;
  char** d = p->b64;
  HIP_TRY(read_back(s, {{fields_b64[0], d[0], nc}, {fields_b64[1], d[1], nc}, {fields_b64[2], d[2], nc},
                        {fields_b64[3], d[3], nc}, {fields_b64[4], d[4], nc}}));
  p->finished = true;
  return AMPH_OK;
}

// ---- device mode ------------------------------------------------------------------
int amph_party_begin_dev(amph_ctx* c, const uint8_t* share_data, size_t share_stride, const uint8_t* masks,
                         const uint8_t* triples, size_t words, int n_parties, uint8_t* oy, uint8_t* orr,
                         uint8_t* ov, void* stream, amph_party** out) {
  if (int st = party_args(c, share_stride, n_parties, words, share_data, masks, triples, out)) return st;
  if (!c->sub.empty()) return fail(AMPH_E_PARAM, "device-mode sessions need a single-device context");
  if (int st = check_dev_words({share_data, masks, triples, oy, orr, ov})) return st;
  HIP_TRY(use_device(c->device));
  std::lock_guard<std::mutex> g(c->mu);
  std::unique_ptr<amph_party> p(new amph_party);
  p->c = c;
  p->W = words;
  p->n = n_parties;
  p->dev = true;
  p->dstream = (hipStream_t)stream;
  uint8_t* const yrv[3] = {oy, orr, ov};
  if (int st = party_alloc(p.get(), false, yrv)) return st;
  p->triples = (const uint4*)triples;
  if (int st = party_pre(p.get(), share_data, share_stride, masks, p->dstream)) return st;
  p->have = 1u;
  *out = p.release();
  return AMPH_OK;
}

int amph_party_text_dev(amph_party* p, const char** text, const uint64_t** len) {
  if (!p || !p->c) return fail(AMPH_E_PARAM, "null party session");
  if (int st = party_mode(p, true)) return st;
  if (!text || !len) return fail(AMPH_E_PARAM, "null output");
  *text = p->text;
  *len = (const uint64_t*)p->text_len_dev;
  return AMPH_OK;
}

int amph_party_partner_dev(amph_party* p, int slot, const char* text, size_t len, int64_t* bad_index,
                           void* stream) {
  if (int st = party_slot_check(p, slot, text, len)) return st;
  if (int st = party_mode(p, true)) return st;
  if (!bad_index || ((uintptr_t)bad_index & 7)) return fail(AMPH_E_PARAM, "bad_index must be an 8-byte aligned device word");
  amph_ctx* c = p->c;
  HIP_TRY(use_device(c->device));
  std::lock_guard<std::mutex> g(c->mu);
  p->dstream = (hipStream_t)stream;
  if (dev_ensure(c, p->verdicts, sizeof(unsigned long long) * AMPH_MAX_PARTIES) != hipSuccess)
    return fail(AMPH_E_NOMEM, "partner verdict words");
  if (!p->partner_ev[slot]) HIP_TRY(hipEventCreateWithFlags(&p->partner_ev[slot], hipEventDisableTiming));
  if (int st = party_decode(p, slot, text, len, (unsigned long long*)bad_index, p->dstream)) return st;
  // the session's copy of the verdict: the caller's word may be reused once
  // the stream has passed this call
  unsigned long long* mine = (unsigned long long*)p->verdicts.p + slot;
  HIP_TRY(hipMemcpyAsync(mine, bad_index, sizeof(unsigned long long), hipMemcpyDeviceToDevice, p->dstream));
  HIP_TRY(hipEventRecord(p->partner_ev[slot], p->dstream));
  p->have |= 1u << slot;
  p->bad_dev[slot] = mine;
  return AMPH_OK;
}

int amph_party_reset_partner(amph_party* p, int slot) {
  if (int st = party_check(p)) return st;
  if (slot < 1 || slot >= p->n)
    return fail(AMPH_E_PARAM, "partner slot must be in [1, " + std::to_string(p->n - 1) + "]");
  std::lock_guard<std::mutex> g(p->c->mu);
  p->have &= ~(1u << slot);
  p->bad_dev[slot] = nullptr;
  return AMPH_OK;
}

int amph_party_finish_b64_dev(amph_party* p, int is_player0, const char* fields_b64[5], void* stream) {
  if (int st = party_check(p)) return st;
  if (int st = party_mode(p, true)) return st;
  if (!fields_b64) return fail(AMPH_E_PARAM, "null field array");
  amph_ctx* c = p->c;
  HIP_TRY(use_device(c->device));
  std::lock_guard<std::mutex> g(c->mu);
  p->dstream = (hipStream_t)stream;
  // every accepted partner call's decode and verdict copy, whatever its stream
  for (int j = 1; j < p->n; ++j)
    if (p->bad_dev[j] && p->partner_ev[j]) HIP_TRY(hipStreamWaitEvent(p->dstream, p->partner_ev[j], 0));
  if (int st = party_open_post(p, is_player0, p->dstream)) return st;
  if (int st = party_b64(p, p->dstream)) return st;
  amph::PoisonB64 pz{};
  for (int j = 1; j < p->n; ++j)
    if (p->bad_dev[j]) pz.bad[pz.n_bad++] = p->bad_dev[j];
  for (int k = 0; k < 5; ++k) pz.field[k] = p->b64[k];
  pz.chars = b64_chars(16 * p->W);
  if (hipError_t e = amph::launch_poison_b64(pz, p->dstream)) return hip_fail(e, "k_poison_b64");
  for (int k = 0; k < 5; ++k) fields_b64[k] = p->b64[k];
  p->finished = true;
  return AMPH_OK;
}

void amph_party_free(amph_party* p) {
  if (!p) return;
  if (p->c) {
    (void)use_device(p->c->device);
    std::lock_guard<std::mutex> g(p->c->mu);
    if (p->dev) (void)hipStreamSynchronize(p->dstream);
    else if (p->c->streams[0]) (void)hipStreamSynchronize(p->c->streams[0]);
    // the buffers go back to the context for the next session
    for (DevBuf* b : {&p->mem, &p->tmp, &p->io}) pool_put(p->c, *b);
    for (DevBuf& b : p->pbuf) pool_put(p->c, b);
  }
  delete p;
}

}  // extern "C"
