// C ABI of libamphora_hip (declared in include/amphora_party_batch.h): many
// Output Delivery requests of one party in one device-resident session.
#include "capi_internal.hpp"
#include "partytiles.hpp"
#include "wiretiles.hpp"

// Device memory: one allocation carved into the triples (host mode), the five
// ODO fields, this party's diffs, the text buffer, the encoder's scratch, the
// five base64 field buffers, the tables (word, pair, text and field offsets,
// the texts' lengths, the reject words) and one row of verdict words per
// partner slot; the share data and masks live in a second one released once
// begin has run (host mode); each partner's span form, pair-order rows,
// windows, scan scratch and (host mode) text lengths in one allocation per
// slot; the partner texts staged in a fourth (host mode).  Host mode: every
// copy is a blocking hipMemcpy issued with the context's stream idle
// (kPageableRule).  Device mode: the caller's buffers are used in place, every
// launch goes on the caller's stream, and the offset tables go up by one
// hipMemcpyAsync from a page-locked image the session allocates at begin and
// frees with itself (a known cost of a device-mode begin: one hipHostMalloc of
// 32 bytes per object).
struct amph_parties {
  amph_ctx* c = nullptr;
  size_t K = 0, T = 0;
  int n = 0;
  bool dev = false;
  hipStream_t dstream = nullptr;  // device mode: the stream of the latest call
  std::vector<uint64_t> woff, toff, foff;  // word (K + 1), text (K) and field (K) offsets
  std::vector<uint64_t> lens;              // host mode: this party's text lengths
  size_t text_bytes = 0, field_chars = 0;
  DevBuf mem, tmp, io;
  DevBuf pbuf[AMPH_MAX_PARTIES];
  amph::PinnedBuf tables_host;  // device mode: the image the tables are uploaded from
  const uint4* triples = nullptr;
  uint4* f5[5] = {};
  char* b64[5] = {};
  uint4* mag0 = nullptr;
  uint8_t* neg0 = nullptr;
  char* text = nullptr;
  void* enc_scratch = nullptr;
  // device tables, contiguous in this order (one upload): word, pair, text, field offsets
  uint64_t *d_woff = nullptr, *d_poff = nullptr, *d_toff = nullptr, *d_foff = nullptr;
  unsigned long long *d_lens = nullptr, *d_reject = nullptr;
  unsigned long long* d_verdict[AMPH_MAX_PARTIES] = {};  // the session's own verdict words per slot
  amph::XSpansSeg xs[AMPH_MAX_PARTIES] = {};
  void* xscratch[AMPH_MAX_PARTIES] = {};
  uint64_t* d_plens[AMPH_MAX_PARTIES] = {};  // host mode: the partner's text lengths
  std::vector<int64_t> verdict_h[AMPH_MAX_PARTIES];  // host mode: the slot's verdicts as reported
  hipEvent_t partner_ev[AMPH_MAX_PARTIES] = {};
  uint32_t have = 0;  // bit j: party j's diffs are on the device (bit 0 after begin)
  bool finished = false;
  ~amph_parties() {
    mem.release();
    tmp.release();
    io.release();
    tables_host.release();
    for (DevBuf& b : pbuf) b.release();
    for (hipEvent_t& e : partner_ev)
      if (e) (void)hipEventDestroy(e);
  }
};

namespace {
size_t table_bytes(size_t K) { return 8 * (4 * K + 2); }  // word, pair (K + 1 each), text, field (K each)

int parties_check(amph_parties* p) {
  if (!p || !p->c) return fail(AMPH_E_PARAM, "null party batch session");
  if (p->finished) return fail(AMPH_E_PARAM, "the party batch session is already finished");
  return AMPH_OK;
}

int parties_mode(const amph_parties* p, bool dev) {
  if (p->dev != dev)
    return fail(AMPH_E_PARAM, dev ? "a host-mode party batch session takes the host calls"
                                  : "a device-mode party batch session takes the *_dev calls");
  return AMPH_OK;
}

int parties_args(amph_ctx* c, size_t share_stride, int n_parties, const uint64_t* woff, size_t K,
                 const void* share_data, const void* masks, const void* triples, amph_parties** out) {
  if (!out) return fail(AMPH_E_PARAM, "null session output");
  *out = nullptr;
  if (check_ctx(c)) return AMPH_E_PARAM;
  if (K == 0) return fail(AMPH_E_PARAM, "a party batch session needs at least one object");
  if (!woff) return fail(AMPH_E_PARAM, "null word_offsets");
  if (share_stride != 16 && share_stride != 32) return fail(AMPH_E_PARAM, "share_stride must be 16 or 32");
  if (n_parties < 1 || n_parties > AMPH_MAX_PARTIES) return fail(AMPH_E_PARAM, "n_parties must be in [1, 16]");
  if (woff[0] != 0) return fail(AMPH_E_PARAM, "word_offsets[0] must be 0");
  for (size_t o = 0; o < K; ++o)
    if (woff[o + 1] < woff[o])
      return fail(AMPH_E_PARAM, "word_offsets must be nondecreasing (object " + std::to_string(o) + ")");
  if (woff[K] > ((uint64_t)1 << 40)) return fail(AMPH_E_PARAM, "too many words");
  if (woff[K] && (!share_data || !masks || !triples)) return fail(AMPH_E_PARAM, "null buffer");
  return AMPH_OK;
}

// the host tables and every size that follows from the word counts alone
void parties_layout(amph_parties* p, const uint64_t* woff, size_t K, int n) {
  p->K = K;
  p->T = (size_t)woff[K];
  p->n = n;
  p->woff.assign(woff, woff + K + 1);
  p->toff.resize(K);
  p->foff.resize(K);
  size_t t = 0, f = 0;
  for (size_t o = 0; o < K; ++o) {
    const size_t W = (size_t)(woff[o + 1] - woff[o]);
    p->toff[o] = t;
    p->foff[o] = f;
    t += amph::xseg_slot_chars(2 * W);
    f += amph::wire_slot_chars(W);
  }
  p->text_bytes = t;
  p->field_chars = f;
}

// the session's device memory; yrv[k] non-null: field k lives in the caller's
// device buffer (device mode), else in the session's
int parties_alloc(amph_parties* p, bool copy_triples, uint8_t* const yrv[3]) {
  const size_t T = p->T, K = p->K, P = 2 * T, nc = p->field_chars;
  const size_t sz[] = {copy_triples ? 192 * T : 0, 16 * T, 16 * T, 16 * T, 16 * T, 16 * T, p->text_bytes,
                       amph::xencs_scratch_bytes(P, K), 64 * T, 4 * T, nc, nc, nc, nc, nc, table_bytes(K), 8 * K,
                       8 * K, 8 * K * (size_t)p->n};
  size_t total = 0;
  for (size_t b : sz) total += align256(b ? b : 16);
  if (pool_ensure(p->c, p->mem, total) != hipSuccess) return fail(AMPH_E_NOMEM, "party batch session device memory");
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
  p->enc_scratch = take(sz[7]);
  p->mag0 = (uint4*)take(sz[8]);
  p->neg0 = take(sz[9]);
  for (int k = 0; k < 5; ++k) p->b64[k] = (char*)take(sz[10 + k]);
  p->d_woff = (uint64_t*)take(sz[15]);
  p->d_poff = p->d_woff + K + 1;
  p->d_toff = p->d_poff + K + 1;
  p->d_foff = p->d_toff + K;
  p->d_lens = (unsigned long long*)take(sz[16]);
  p->d_reject = (unsigned long long*)take(sz[17]);
  unsigned long long* v = (unsigned long long*)take(sz[18]);
  for (int j = 0; j < p->n; ++j) p->d_verdict[j] = v + (size_t)j * K;
  return AMPH_OK;
}

// the four offset tables as the device holds them
void parties_table_image(const amph_parties* p, uint64_t* img) {
  const size_t K = p->K;
  for (size_t o = 0; o <= K; ++o) {
    img[o] = p->woff[o];
    img[K + 1 + o] = 2 * p->woff[o];
  }
  for (size_t o = 0; o < K; ++o) {
    img[2 * K + 2 + o] = p->toff[o];
    img[3 * K + 2 + o] = p->foff[o];
  }
}

// k_odo_pre over the T words (y, r, v + this party's diffs), then the K texts
int parties_pre(amph_parties* p, const uint8_t* dshare, size_t share_stride, const uint8_t* dmasks, hipStream_t s) {
  amph_ctx* c = p->c;
  const size_t T = p->T, P = 2 * T;
  hipError_t e = amph::launch_odo_pre((const uint4*)dshare, (int)(share_stride / 16), (const uint4*)dmasks,
                                      p->triples, T, p->f5[0], p->f5[1], p->f5[2], p->mag0, (uint32_t*)p->neg0,
                                      c->f, cfg(c, s, T));
  if (e != hipSuccess) return hip_fail(e, "k_odo_pre");
  e = amph::launch_exchange_encode_seg(p->mag0, p->neg0, P, p->d_poff, p->d_toff, p->K, p->text, p->text_bytes,
                                       p->d_lens, p->enc_scratch, cfg(c, s, P));
  return e == hipSuccess ? AMPH_OK : hip_fail(e, "k_xencs");
}

int parties_slot_check(amph_parties* p, int slot, const void* texts, const void* lens, const void* bad) {
  if (int st = parties_check(p)) return st;
  if (slot < 1 || slot >= p->n)
    return fail(AMPH_E_PARAM, "partner slot must be in [1, " + std::to_string(p->n - 1) + "]");
  if (p->have >> slot & 1u)
    return fail(AMPH_E_PARAM, "partner slot " + std::to_string(slot) + " already holds its texts");
  if (!texts || !lens || !bad) return fail(AMPH_E_PARAM, "null texts, text_lens or bad_index");
  return AMPH_OK;
}

// a partner's K texts (device memory, at the session's offsets) decoded into
// the slot's span form; bad: the K device words the decode reports into
int parties_decode(amph_parties* p, int slot, const char* dtexts, const uint64_t* dlens, unsigned long long* bad,
                   bool host_lens, hipStream_t s) {
  const size_t P = 2 * p->T, K = p->K;
  const size_t nb = amph::xdec_span_grid(p->text_bytes), tiles = amph::party_tile_grid(P, K);
  const size_t xsz[8] = {16 * nb * amph::kPartySpanSlots, nb * amph::kPartySpanSlots, 8 * (nb + 1), 32 * P, 2 * P,
                         16 * tiles, amph::xspans_seg_scratch_bytes(p->text_bytes), host_lens ? 8 * K : 0};
  size_t xtotal = 0;
  for (size_t b : xsz) xtotal += align256(b ? b : 16);
  if (pool_ensure(p->c, p->pbuf[slot], xtotal) != hipSuccess)
    return fail(AMPH_E_NOMEM, "party batch session partner diffs");
  uint8_t* cur = (uint8_t*)p->pbuf[slot].p;
  auto take = [&](size_t b) {
    uint8_t* q = cur;
    cur += align256(b ? b : 16);
    return q;
  };
  amph::XSpansSeg& xs = p->xs[slot];
  xs.mag = (uint4*)take(xsz[0]);
  xs.neg = take(xsz[1]);
  xs.base = (uint64_t*)take(xsz[2]);
  xs.pmag = (uint4*)take(xsz[3]);
  xs.pneg = take(xsz[4]);
  xs.win = (uint4*)take(xsz[5]);
  p->xscratch[slot] = take(xsz[6]);
  p->d_plens[slot] = (uint64_t*)take(xsz[7]);
  xs.nb = nb;
  if (host_lens) {
    hipError_t e = hipMemcpy(p->d_plens[slot], dlens, 8 * K, hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail(e, "text_lens upload");
    dlens = p->d_plens[slot];
  }
  hipError_t e = amph::launch_exchange_decode_spans_seg(dtexts, p->text_bytes, p->d_poff, p->d_toff, dlens, K, P, xs,
                                                        bad, p->xscratch[slot], cfg(p->c, s, p->text_bytes));
  return e == hipSuccess ? AMPH_OK : hip_fail(e, "k_xdecs_span");
}

int parties_all_in(amph_parties* p) {
  const uint32_t all = (1u << p->n) - 1u;
  if ((p->have & all) == all) return AMPH_OK;
  int j = 1;
  while (j < p->n && (p->have >> j & 1u)) ++j;
  return fail(AMPH_E_PARAM, "partner slot " + std::to_string(j) + "'s interimValues texts are missing");
}

// the summed diffs -> w, u on the device, and the reject words
int parties_open_post(amph_parties* p, int is_player0, hipStream_t s) {
  amph::PartySegSet set{};
  set.mag0 = p->mag0;
  set.neg0 = (const uint32_t*)p->neg0;
  for (int j = 1; j < p->n; ++j) {
    set.span[j] = p->xs[j];
    set.verdict[j] = p->d_verdict[j];
  }
  set.pair_offsets = p->d_poff;
  set.text_offsets = p->d_toff;
  set.n_objects = p->K;
  set.npairs = 2 * p->T;
  set.reject = p->d_reject;
  hipError_t e = amph::launch_open_post_seg(set, p->n, p->triples, is_player0, p->f5[3], p->f5[4], p->c->f,
                                            cfg(p->c, s, p->T));
  return e == hipSuccess ? AMPH_OK : hip_fail(e, "k_open_post_seg");
}

// the 5 K field texts in the session's memory (one launch)
int parties_b64(amph_parties* p, hipStream_t s) {
  if (p->T == 0) return AMPH_OK;  // every text is empty
  const uint8_t* const in[5] = {(const uint8_t*)p->f5[0], (const uint8_t*)p->f5[1], (const uint8_t*)p->f5[2],
                                (const uint8_t*)p->f5[3], (const uint8_t*)p->f5[4]};
  hipError_t e = amph::launch_odo_b64_seg(in, p->b64, p->d_woff, p->d_foff, p->K, amph::wire_tile_grid(p->T, p->K),
                                          p->T, p->field_chars, p->d_reject, cfg(p->c, s, p->T));
  return e == hipSuccess ? AMPH_OK : hip_fail(e, "k_odo_b64_seg");
}

}  // namespace

extern "C" {

int amph_parties_begin(amph_ctx* c, const uint8_t* share_data, size_t share_stride, const uint8_t* masks,
                       const uint8_t* triples, const uint64_t* word_offsets, size_t n_objects, int n_parties,
                       uint8_t* oy, uint8_t* orr, uint8_t* ov, amph_parties** out) {
  if (int st = parties_args(c, share_stride, n_parties, word_offsets, n_objects, share_data, masks, triples, out))
    return st;
  c = first_device(c);  // a multi-device context runs sessions on its first device
  HIP_TRY(use_device(c->device));
  std::lock_guard<std::mutex> g(c->mu);
  std::unique_ptr<amph_parties> p(new amph_parties);
  p->c = c;
  parties_layout(p.get(), word_offsets, n_objects, n_parties);
  const size_t T = p->T, K = p->K;
  uint8_t* const none[3] = {nullptr, nullptr, nullptr};
  if (int st = parties_alloc(p.get(), true, none)) return st;
  if (pool_ensure(c, p->tmp, align256(share_stride * T + 16) + align256(64 * T + 16)) != hipSuccess)
    return fail(AMPH_E_NOMEM, "party batch session staging");
  uint8_t* dshare = (uint8_t*)p->tmp.p;
  uint8_t* dmasks = dshare + align256(share_stride * T + 16);
  hipStream_t s;
  if (int st = host_stream(c, 0, &s)) return st;
  HIP_TRY(hipStreamSynchronize(s));
  std::vector<uint64_t> img(table_bytes(K) / 8);
  parties_table_image(p.get(), img.data());
  HIP_TRY(hipMemcpy(p->d_woff, img.data(), table_bytes(K), hipMemcpyHostToDevice));
  // what lies between the texts reads 0 on the host (amph_parties_text, finish_b64)
  HIP_TRY(hipMemsetAsync(p->text, 0, p->text_bytes, s));
  for (int k = 0; k < 5 && p->field_chars; ++k) HIP_TRY(hipMemsetAsync(p->b64[k], 0, p->field_chars, s));
  if (T) {
    HIP_TRY(hipMemcpy(dshare, share_data, share_stride * T, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dmasks, masks, 64 * T, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy((void*)p->triples, triples, 192 * T, hipMemcpyHostToDevice));
  }
  if (int st = parties_pre(p.get(), dshare, share_stride, dmasks, s)) return st;
  p->lens.resize(K);
  HIP_TRY(read_back(s, {{p->lens.data(), p->d_lens, 8 * K}, {oy, p->f5[0], oy ? 16 * T : 0},
                        {orr, p->f5[1], orr ? 16 * T : 0}, {ov, p->f5[2], ov ? 16 * T : 0}}));
  p->have = 1u;
  pool_put(c, p->tmp);
  *out = p.release();
  return AMPH_OK;
}

size_t amph_parties_objects(const amph_parties* p) { return p ? p->K : 0; }
size_t amph_parties_words(const amph_parties* p) { return p ? p->T : 0; }
size_t amph_parties_text_bytes(const amph_parties* p) { return p ? p->text_bytes : 0; }
size_t amph_parties_field_chars(const amph_parties* p) { return p ? p->field_chars : 0; }

int amph_parties_text_offsets(const amph_parties* p, uint64_t* out) {
  if (!p || !out) return fail(AMPH_E_PARAM, "null party batch session or output");
  std::copy(p->toff.begin(), p->toff.end(), out);
  return AMPH_OK;
}

int amph_parties_field_offsets(const amph_parties* p, uint64_t* out) {
  if (!p || !out) return fail(AMPH_E_PARAM, "null party batch session or output");
  std::copy(p->foff.begin(), p->foff.end(), out);
  return AMPH_OK;
}

int amph_parties_text_lens(amph_parties* p, uint64_t* out) {
  if (!p || !p->c) return fail(AMPH_E_PARAM, "null party batch session");
  if (int st = parties_mode(p, false)) return st;
  if (!out) return fail(AMPH_E_PARAM, "null output");
  std::copy(p->lens.begin(), p->lens.end(), out);
  return AMPH_OK;
}

int amph_parties_text(amph_parties* p, size_t object, char* out, size_t out_cap) {
  if (!p || !p->c) return fail(AMPH_E_PARAM, "null party batch session");
  if (int st = parties_mode(p, false)) return st;
  if (object != AMPH_PARTIES_ALL && object >= p->K)
    return fail(AMPH_E_RANGE, "object " + std::to_string(object) + " of " + std::to_string(p->K));
  const size_t at = object == AMPH_PARTIES_ALL ? 0 : (size_t)p->toff[object];
  const size_t len = object == AMPH_PARTIES_ALL ? p->text_bytes : (size_t)p->lens[object];
  if (!out && len) return fail(AMPH_E_PARAM, "null output");
  if (out_cap < len)
    return fail(AMPH_E_LEN, "output capacity " + std::to_string(out_cap) + " below the text length " +
                                std::to_string(len));
  amph_ctx* c = p->c;
  HIP_TRY(use_device(c->device));
  std::lock_guard<std::mutex> g(c->mu);
  hipStream_t s;
  if (int st = host_stream(c, 0, &s)) return st;
  HIP_TRY(read_back(s, {{out, p->text + at, len}}));
  return AMPH_OK;
}

int amph_parties_partner(amph_parties* p, int slot, const char* texts, const uint64_t* text_lens,
                         int64_t* bad_index) {
  if (int st = parties_slot_check(p, slot, texts, text_lens, bad_index)) return st;
  if (int st = parties_mode(p, false)) return st;
  const size_t K = p->K;
  size_t used = 0;
  for (size_t o = 0; o < K; ++o) {
    const size_t room = (size_t)((o + 1 < K ? p->toff[o + 1] : p->text_bytes) - p->toff[o]);
    if (text_lens[o] > room)
      return fail(AMPH_E_PARAM, "object " + std::to_string(o) + ": a text of " + std::to_string(text_lens[o]) +
                                    " characters runs past its slot of " + std::to_string(room));
    if (text_lens[o]) used = (size_t)(p->toff[o] + text_lens[o]);
  }
  for (size_t o = 0; o < K; ++o) bad_index[o] = -1;
  amph_ctx* c = p->c;
  HIP_TRY(use_device(c->device));
  std::lock_guard<std::mutex> g(c->mu);
  if (pool_ensure(c, p->io, align256(p->text_bytes + 16)) != hipSuccess)
    return fail(AMPH_E_NOMEM, "party batch session text staging");
  char* dtexts = (char*)p->io.p;
  hipStream_t s;
  if (int st = host_stream(c, 0, &s)) return st;
  HIP_TRY(hipStreamSynchronize(s));
  if (used) HIP_TRY(hipMemcpy(dtexts, texts, used, hipMemcpyHostToDevice));
  if (int st = parties_decode(p, slot, dtexts, text_lens, p->d_verdict[slot], true, s)) return st;
  std::vector<int64_t>& v = p->verdict_h[slot];
  v.assign(K, -1);
  HIP_TRY(read_back(s, {{v.data(), p->d_verdict[slot], 8 * K}}));
  p->have |= 1u << slot;
  size_t nbad = 0, nlen = 0, fb = 0, fl = 0;
  for (size_t o = 0; o < K; ++o) {
    if (v[o] == (int64_t)AMPH_NO_FAILURE) {
      v[o] = -1;
      continue;
    }
    bad_index[o] = v[o];
    if ((uint64_t)v[o] == text_lens[o]) {
      if (!nlen++) fl = o;
    } else if (!nbad++) {
      fb = o;
    }
  }
  if (nbad)
    return fail(AMPH_E_PARAM, "object " + std::to_string(fb) + ": Malformed FactorPair JSON at offset " +
                                  std::to_string(v[fb]) + " (" + std::to_string(nbad + nlen) + " of " +
                                  std::to_string(K) + " texts refused)");
  if (nlen)
    return fail(AMPH_E_LEN, "object " + std::to_string(fl) + ": interimValues must hold exactly " +
                                std::to_string(2 * (p->woff[fl + 1] - p->woff[fl])) + " FactorPairs (" +
                                std::to_string(nlen) + " of " + std::to_string(K) + " texts refused)");
  return AMPH_OK;
}

int amph_parties_reset_partner(amph_parties* p, int slot) {
  if (int st = parties_check(p)) return st;
  if (slot < 1 || slot >= p->n)
    return fail(AMPH_E_PARAM, "partner slot must be in [1, " + std::to_string(p->n - 1) + "]");
  std::lock_guard<std::mutex> g(p->c->mu);
  p->have &= ~(1u << slot);
  p->verdict_h[slot].clear();
  return AMPH_OK;
}

int amph_parties_finish(amph_parties* p, int is_player0, uint8_t* ow, uint8_t* ou) {
  if (int st = parties_check(p)) return st;
  if (int st = parties_mode(p, false)) return st;
  if (p->T && (!ow || !ou)) return fail(AMPH_E_PARAM, "null output");
  if (int st = parties_all_in(p)) return st;
  amph_ctx* c = p->c;
  HIP_TRY(use_device(c->device));
  std::lock_guard<std::mutex> g(c->mu);
  hipStream_t s;
  if (int st = host_stream(c, 0, &s)) return st;
  if (int st = parties_open_post(p, is_player0, s)) return st;
  HIP_TRY(read_back(s, {{ow, p->f5[3], 16 * p->T}, {ou, p->f5[4], 16 * p->T}}));
  p->finished = true;
  return AMPH_OK;
}

int amph_parties_finish_b64(amph_parties* p, int is_player0, char* const fields_b64[5], uint8_t* rejected) {
  if (int st = parties_check(p)) return st;
  if (int st = parties_mode(p, false)) return st;
  if (!fields_b64) return fail(AMPH_E_PARAM, "null field array");
  for (int k = 0; k < 5; ++k)
    if (p->field_chars && !fields_b64[k]) return fail(AMPH_E_PARAM, "null field text");
  if (int st = parties_all_in(p)) return st;
  amph_ctx* c = p->c;
  HIP_TRY(use_device(c->device));
  std::lock_guard<std::mutex> g(c->mu);
  hipStream_t s;
  if (int st = host_stream(c, 0, &s)) return st;
  if (int st = parties_open_post(p, is_player0, s)) return st;
  if (int st = parties_b64(p, s)) return st;
  const size_t nc = p->field_chars;
  char** d = p->b64;
  HIP_TRY(read_back(s, {{fields_b64[0], d[0], nc}, {fields_b64[1], d[1], nc}, {fields_b64[2], d[2], nc},
                        {fields_b64[3], d[3], nc}, {fields_b64[4], d[4], nc}}));
  if (rejected)
    for (size_t o = 0; o < p->K; ++o) {
      rejected[o] = 0;
      for (int j = 1; j < p->n; ++j) rejected[o] |= p->verdict_h[j][o] >= 0;
    }
  p->finished = true;
  return AMPH_OK;
}

// ---- device mode ------------------------------------------------------------------
int amph_parties_begin_dev(amph_ctx* c, const uint8_t* share_data, size_t share_stride, const uint8_t* masks,
                           const uint8_t* triples, const uint64_t* word_offsets, size_t n_objects, int n_parties,
                           uint8_t* oy, uint8_t* orr, uint8_t* ov, void* stream, amph_parties** out) {
  if (int st = parties_args(c, share_stride, n_parties, word_offsets, n_objects, share_data, masks, triples, out))
    return st;
  if (!c->sub.empty()) return fail(AMPH_E_PARAM, "device-mode sessions need a single-device context");
  if (int st = check_dev_words({share_data, masks, triples, oy, orr, ov})) return st;
  HIP_TRY(use_device(c->device));
  std::lock_guard<std::mutex> g(c->mu);
  std::unique_ptr<amph_parties> p(new amph_parties);
  p->c = c;
  p->dev = true;
  p->dstream = (hipStream_t)stream;
  parties_layout(p.get(), word_offsets, n_objects, n_parties);
  uint8_t* const yrv[3] = {oy, orr, ov};
  if (int st = parties_alloc(p.get(), false, yrv)) return st;
  p->triples = (const uint4*)triples;
  if (p->tables_host.ensure(table_bytes(p->K)) != hipSuccess)
    return fail(AMPH_E_NOMEM, "party batch session page-locked tables");
  parties_table_image(p.get(), (uint64_t*)p->tables_host.p);
  hipError_t e = hipMemcpyAsync(p->d_woff, p->tables_host.p, table_bytes(p->K), hipMemcpyHostToDevice, p->dstream);
  int st = e == hipSuccess ? parties_pre(p.get(), share_data, share_stride, masks, p->dstream)
                           : hip_fail(e, "offset tables upload");
  if (st) {  // the upload may be in flight: its source is freed only after the stream
    (void)hipStreamSynchronize(p->dstream);
    pool_put(c, p->mem);
    return st;
  }
  p->have = 1u;
  *out = p.release();
  return AMPH_OK;
}

int amph_parties_text_dev(amph_parties* p, const char** texts, const uint64_t** text_offsets,
                          const uint64_t** text_lens) {
  if (!p || !p->c) return fail(AMPH_E_PARAM, "null party batch session");
  if (int st = parties_mode(p, true)) return st;
  if (!texts || !text_offsets || !text_lens) return fail(AMPH_E_PARAM, "null output");
  *texts = p->text;
  *text_offsets = p->d_toff;
  *text_lens = (const uint64_t*)p->d_lens;
  return AMPH_OK;
}

int amph_parties_partner_dev(amph_parties* p, int slot, const char* texts, const uint64_t* text_lens,
                             int64_t* bad_index, void* stream) {
  if (int st = parties_slot_check(p, slot, texts, text_lens, bad_index)) return st;
  if (int st = parties_mode(p, true)) return st;
  if ((uintptr_t)texts & 15) return fail(AMPH_E_PARAM, "the text buffer must be 16-byte aligned");
  if (((uintptr_t)text_lens & 7) || ((uintptr_t)bad_index & 7))
    return fail(AMPH_E_PARAM, "text_lens and bad_index must be 8-byte aligned device arrays");
  amph_ctx* c = p->c;
  HIP_TRY(use_device(c->device));
  std::lock_guard<std::mutex> g(c->mu);
  p->dstream = (hipStream_t)stream;
  if (!p->partner_ev[slot]) HIP_TRY(hipEventCreateWithFlags(&p->partner_ev[slot], hipEventDisableTiming));
  if (int st = parties_decode(p, slot, texts, text_lens, (unsigned long long*)bad_index, false, p->dstream))
    return st;
  // the session's copy of the verdicts: the caller's array may be reused once
  // the stream has passed this call
  HIP_TRY(hipMemcpyAsync(p->d_verdict[slot], bad_index, 8 * p->K, hipMemcpyDeviceToDevice, p->dstream));
  HIP_TRY(hipEventRecord(p->partner_ev[slot], p->dstream));
  p->have |= 1u << slot;
  return AMPH_OK;
}

int amph_parties_finish_b64_dev(amph_parties* p, int is_player0, const char* fields_b64[5], void* stream) {
  if (int st = parties_check(p)) return st;
  if (int st = parties_mode(p, true)) return st;
  if (!fields_b64) return fail(AMPH_E_PARAM, "null field array");
  if (int st = parties_all_in(p)) return st;
  amph_ctx* c = p->c;
  HIP_TRY(use_device(c->device));
  std::lock_guard<std::mutex> g(c->mu);
  p->dstream = (hipStream_t)stream;
  // every accepted partner call's decode and verdict copy, whatever its stream
  for (int j = 1; j < p->n; ++j)
    if (p->partner_ev[j]) HIP_TRY(hipStreamWaitEvent(p->dstream, p->partner_ev[j], 0));
  if (int st = parties_open_post(p, is_player0, p->dstream)) return st;
  if (int st = parties_b64(p, p->dstream)) return st;
  for (int k = 0; k < 5; ++k) fields_b64[k] = p->b64[k];
  p->finished = true;
  return AMPH_OK;
}

void amph_parties_free(amph_parties* p) {
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
