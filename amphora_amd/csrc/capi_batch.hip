// C ABI of libamphora_hip: the many-objects-per-call families --
// include/amphora_wire_batch.h (K_RV / K_MASK from K objects' wire texts),
// include/amphora_upload_batch.h (K MaskedInput uploads, both ends),
// include/amphora_respond_batch.h (K Output Delivery responses' fields) and
// include/amphora_exchange_batch.h (K requests' Beaver exchange texts).
#include "capi_internal.hpp"
#include "wiretiles.hpp"
#include "respondtiles.hpp"
#include "exchangetiles.hpp"

namespace {
// (the host image every call here moves, BatchImage, and the wire-text calls'
// wire_batch_status live in capi_internal.hpp: clients_session.hip shares them)

// ---- the host tables of the packed calls -------------------------------------------
// starts at 0, never decreases
int check_word_table(const uint64_t* woff, size_t K) {
  if (woff[0] != 0) return fail(AMPH_E_PARAM, "word_offsets[0] must be 0");
  for (size_t o = 0; o < K; ++o)
    if (woff[o + 1] < woff[o])
      return fail(AMPH_E_PARAM, "word_offsets must not decrease (entry " + std::to_string(o + 1) + ")");
  return AMPH_OK;
}

// Where the objects' texts lie in a buffer: object o's chars(W_o) characters
// at off[o] end before the capacity; a slotted table's entries are multiples
// of 16 and a text ends before the next slot too.
struct TextRule {
  const char* table;  // the slotted table's name; null: any alignment, the capacity alone
  const char* what;   // the text in the message
  size_t (*chars)(size_t words);
  const char *cap_pre, *cap_post;  // around the capacity in the message
};
const TextRule kWireSlots = {"text_offsets", "text", amph::wire_text_chars, "the buffers' ", " characters"};
const TextRule kFramedSlots = {"out_text_offsets", "output text", amph::masked_input_data_chars,
                               "the output capacity ", ""};
const TextRule kUploadTexts = {nullptr, "text", amph::masked_input_data_chars, "the ", " characters of the texts"};

int check_texts(const TextRule& r, const uint64_t* woff, const uint64_t* off, size_t K, uint64_t cap) {
  for (size_t o = 0; o < K; ++o) {
    const uint64_t end = off[o] + r.chars(woff[o + 1] - woff[o]);
    const bool next = r.table && o + 1 < K;
    if (r.table && off[o] % 16)
      return fail(AMPH_E_PARAM, std::string(r.table) + "[" + std::to_string(o) + "] = " + std::to_string(off[o]) +
                                    " must be a multiple of 16");
    if (end < off[o] || end > (next ? off[o + 1] : cap))
      return fail(AMPH_E_PARAM, "object " + std::to_string(o) + ": its " + r.what + " [" + std::to_string(off[o]) +
                                    ", " + std::to_string(end) + ") runs past " +
                                    (next ? "the next slot at " + std::to_string(off[o + 1])
                                          : r.cap_pre + std::to_string(cap) + r.cap_post));
  }
  return AMPH_OK;
}

// the host tables of a packed wire call against the buffers' length
int check_wire_tables(const uint64_t* woff, const uint64_t* toff, size_t K, size_t nchars) {
  if (int st = check_word_table(woff, K)) return st;
  return check_texts(kWireSlots, woff, toff, K, nchars);
}

int tables_misaligned(std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs)
    if ((uintptr_t)p & 7)
      return fail(AMPH_E_PARAM, "device offset tables and verdict arrays must be 8-byte aligned");
  return AMPH_OK;
}

// device mode: the caller's verdict arrays to the sentinel on its stream,
// unless it accumulates (AMPH_F_ACCUMULATE: min-combine into them)
int reset_verdicts_dev(std::initializer_list<int64_t*> arrays, size_t K, uint32_t flags, hipStream_t s) {
  if (flags & AMPH_F_ACCUMULATE) return AMPH_OK;
  for (int64_t* v : arrays) HIP_TRY(hipMemsetAsync(v, 0x7F, 8 * K, s));
  return AMPH_OK;
}

// ---- K_RV / K_MASK from the wire, many objects per call -------------------------
// include/amphora_wire_batch.h: the slotted text layout (wire.hip,
// wiretiles.hpp).  The image: [word table | text table | 5 n field buffers |
// secrets] in, [16-byte words | records | 2 K verdict words] out.

// How a host call's pieces enter and leave the image: text(j, k, o) = party
// j's field k of object o (nchars_o characters), secrets(o) / out16(o) /
// out24(o) = object o's words (null: not wanted), out_text(o) = object o's
// framed "data" array text (amphora_upload_batch.h).
struct WirePieces {
  std::function<const char*(int, int, size_t)> text;
  std::function<const uint8_t*(size_t)> secrets;
  std::function<uint8_t*(size_t)> out16;
  std::function<char*(size_t)> out24;
  std::function<char*(size_t)> out_text;
};

// Host mode of all four calls, tables validated: woff[K + 1], toff[K] (a
// field buffer of the image holds `chars` characters).  framed (the mask
// calls of amphora_upload_batch.h): the output is every object's framed text
// instead, in the image's own dense 16-byte-aligned slots; the copies count
// into upload_copies.
int wire_batch_host(amph_ctx* c, int n, size_t K, const uint64_t* woff, const uint64_t* toff, size_t chars,
                    bool masked, bool want16, bool want24, const WirePieces& io, int64_t* first_fail,
                    int64_t* bad_char, bool framed = false) {
  const size_t T = woff[K];
  for (size_t o = 0; o < K; ++o) first_fail[o] = bad_char[o] = -1;
  if (T == 0) {
    for (size_t o = 0; framed && o < K; ++o) std::memcpy(io.out_text(o), "[]", 2);
    return AMPH_OK;
  }
  const size_t fchars = align256(chars ? chars : 16);
  size_t ochars = 0;  // the framed texts' slots: object o's at the sum of its predecessors' strides
  for (size_t o = 0; framed && o < K; ++o) ochars += amph::upload_slot_chars(woff[o + 1] - woff[o]);
  BatchImage m;
  const size_t tab_w = m.in(8 * (K + 1)), tab_t = m.in(8 * K), tab_o = m.in(framed ? 8 * K : 0);
  const size_t txt = m.in(5 * (size_t)n * fchars), sec = m.in(masked ? 16 * T : 0);
  const size_t o16 = m.out(want16 ? 16 * T : 0), o24 = m.out(want24 ? 24 * T : 0), otx = m.out(ochars);
  m.verdicts(2 * K, "verdict arrays");
  if (int st = m.open(c, framed ? &amph_ctx::upload_copies : &amph_ctx::wire_copies, "wire")) return st;
  std::memcpy(m.host(tab_w), woff, 8 * (K + 1));
  std::memcpy(m.host(tab_t), toff, 8 * K);
  uint64_t* ooff = (uint64_t*)m.host(tab_o);
  for (size_t o = 0, at = 0; framed && o < K; ++o) {
    ooff[o] = at;
    at += amph::upload_slot_chars(woff[o + 1] - woff[o]);
  }
  amph::TextSet tx{};
  for (int j = 0; j < n; ++j)
    for (int k = 0; k < 5; ++k) {
      const size_t at = txt + (size_t)(5 * j + k) * fchars;
      for (size_t o = 0; o < K; ++o)
        if (const size_t nc = amph::wire_text_chars(woff[o + 1] - woff[o]))
          std::memcpy(m.host(at + toff[o]), io.text(j, k, o), nc);
      tx.t[k][j] = (const char*)m.dev(at);
    }
  for (size_t o = 0; masked && o < K; ++o)
    if (woff[o + 1] > woff[o]) std::memcpy(m.host(sec + 16 * woff[o]), io.secrets(o), 16 * (woff[o + 1] - woff[o]));
  if (int st = m.upload()) return st;
  const uint64_t *dw = m.dev_table(tab_w), *dt = m.dev_table(tab_t);
  unsigned long long *dff = m.dverd, *dbad = m.dverd + K;
  const size_t grid = amph::wire_tile_grid(T, K);
  const amph::LaunchCfg lc = cfg(m.c, m.s, T);
  hipError_t e =
      framed ? amph::launch_mask_json_seg(tx, n, dw, dt, m.dev_table(tab_o), K, grid, (const uint4*)m.dev(sec),
                                          (char*)m.dev(otx), dff, dbad, m.c->f, lc)
      : masked ? amph::launch_mask_b64_seg(tx, n, dw, dt, K, grid, (const uint4*)m.dev(sec),
                                           want16 ? (uint4*)m.dev(o16) : nullptr,
                                           want24 ? (char*)m.dev(o24) : nullptr, dff, dbad, m.c->f, lc)
             : amph::launch_rv_b64_seg(tx, n, dw, dt, K, grid, (uint4*)m.dev(o16), dff, dbad, m.c->f, lc);
  if (int st = m.finish(e, framed ? "k_mask_json_seg" : masked ? "k_mask_b64_seg" : "k_rv_b64_seg")) return st;
  for (size_t o = 0; o < K; ++o) {
    const size_t w0 = woff[o], w = woff[o + 1] - w0;
    if (framed) std::memcpy(io.out_text(o), m.host(otx + ooff[o]), amph::masked_input_data_chars(w));
    if (!w) continue;
    if (want16) std::memcpy(io.out16(o), m.host(o16 + 16 * w0), 16 * w);
    if (want24) std::memcpy(io.out24(o), m.host(o24 + 24 * w0), 24 * w);
  }
  return wire_batch_status(m.verdict_words(), K, woff, first_fail, bad_char);
}

// The framed form of a packed call (amph_mask_input_json_packed): object o's
// "data" array text goes to text[ooff[o]:] instead of out16 / out24.
struct FramedOut {
  const uint64_t* ooff;
  char* text;
  size_t cap;
};

// All three packed calls: `masked` = false runs K_RV (out16 = the secrets out).
int wire_packed_call(amph_ctx* c, const amph_odo_b64* odos, int n, const uint64_t* woff, const uint64_t* toff,
                     size_t K, bool masked, const uint8_t* secrets, uint8_t* out16, char* out24,
                     int64_t* first_fail, int64_t* bad_char, uint32_t flags, void* stream,
                     const FramedOut* fr = nullptr) {
  if (check_ctx(c)) return AMPH_E_PARAM;
  AMPH_NO_HOST_IO(flags);
  if (K == 0) return AMPH_OK;
  if (int st = check_parties(odos, n)) return st;
  if (fr ? !woff || !toff || !fr->ooff || !fr->text || !first_fail || !bad_char
         : !woff || !toff || !first_fail || !bad_char)
    return fail(AMPH_E_PARAM, fr ? "null offsets table, output text or verdict array"
                                 : "null offsets table or verdict array");
  for (int j = 1; j < n; ++j)
    if (odos[j].nchars != odos[0].nchars)
      return fail(AMPH_E_LEN, "party " + std::to_string(j) + ": field buffers of " + std::to_string(odos[j].nchars) +
                                  " characters, party 0's hold " + std::to_string(odos[0].nchars));
  const size_t nchars = odos[0].nchars;
  const bool no_io = fr ? !secrets : (!masked && !out16) || (masked && !secrets);
  const char* const no_io_msg = fr ? "null secrets" : "null secrets/output";
  if (flags & AMPH_F_DEVICE) {
    amph::TextSet tx{};
    for (int j = 0; j < n; ++j)
      for (int k = 0; k < 5; ++k) {
        tx.t[k][j] = b64_field(odos[j], k);
        if (nchars && !tx.t[k][j]) return fail(AMPH_E_PARAM, "null ODO field text");
        if (int st = check_dev_words({tx.t[k][j]})) return st;
      }
    if (int st = check_dev_words({secrets, out16, out24, fr ? fr->text : nullptr})) return st;
    if (int st = tables_misaligned({woff, toff, fr ? fr->ooff : nullptr, first_fail, bad_char})) return st;
    if (nchars && no_io) return fail(AMPH_E_PARAM, no_io_msg);
    c = first_device(c);
    HIP_TRY(use_device(c->device));
    hipStream_t s = (hipStream_t)stream;
    if (int st = reset_verdicts_dev({first_fail, bad_char}, K, flags, s)) return st;
    // the word table is the device's: every text of W words takes at least
    // 64 W / 3 characters of the buffers, so T <= 3 nchars / 64 bounds the
    // grid (the surplus workgroups find no tile and exit)
    const size_t tbound = 3 * (nchars / 64) + 3, grid = amph::wire_tile_grid(tbound, K);
    // the framed launch runs for nchars == 0 too: every object is empty and gets its "[]"
    if (nchars == 0 && !fr) return AMPH_OK;
    unsigned long long *dff = (unsigned long long*)first_fail, *dbad = (unsigned long long*)bad_char;
    const amph::LaunchCfg lc = cfg(c, s, tbound);
    hipError_t e = fr ? amph::launch_mask_json_seg(tx, n, woff, toff, fr->ooff, K, grid, (const uint4*)secrets,
                                                   fr->text, dff, dbad, c->f, lc)
                   : masked ? amph::launch_mask_b64_seg(tx, n, woff, toff, K, grid, (const uint4*)secrets,
                                                        (uint4*)out16, out24, dff, dbad, c->f, lc)
                            : amph::launch_rv_b64_seg(tx, n, woff, toff, K, grid, (uint4*)out16, dff, dbad, c->f, lc);
    return e == hipSuccess ? AMPH_OK
                           : hip_fail(e, fr ? "k_mask_json_seg" : masked ? "k_mask_b64_seg" : "k_rv_b64_seg");
  }
  if (int st = check_wire_tables(woff, toff, K, nchars)) return st;
  if (fr)
    if (int st = check_texts(kFramedSlots, woff, fr->ooff, K, fr->cap)) return st;
  const size_t T = woff[K];
  if (T) {
    for (int j = 0; j < n; ++j)
      for (int k = 0; k < 5; ++k)
        if (!b64_field(odos[j], k)) return fail(AMPH_E_PARAM, "null ODO field text");
    if (no_io) return fail(AMPH_E_PARAM, no_io_msg);
  }
  WirePieces io;
  io.text = [&](int j, int k, size_t o) { return b64_field(odos[j], k) + toff[o]; };
  io.secrets = [&](size_t o) { return secrets + 16 * woff[o]; };
  io.out16 = [&](size_t o) { return out16 + 16 * woff[o]; };
  io.out24 = [&](size_t o) { return out24 + 24 * woff[o]; };
  io.out_text = [&](size_t o) { return fr->text + fr->ooff[o]; };
  const size_t used = toff[K - 1] + amph::wire_text_chars(woff[K] - woff[K - 1]);  // the last text's end
  return wire_batch_host(c, n, K, woff, toff, used, masked, out16 != nullptr, out24 != nullptr, io, first_fail,
                         bad_char, fr != nullptr);
}

// The gathered calls: odos[o * n + j], one words[o] per object.  out_texts
// (amph_mask_input_json_batch): the framed texts instead of out16 / out24.
int wire_batch_call(amph_ctx* c, const amph_odo_b64* odos, int n, size_t K, const size_t* words, bool masked,
                    const uint8_t* const* secrets, uint8_t* const* out16, char* const* out24,
                    int64_t* first_fail, int64_t* bad_char, uint32_t flags, char* const* out_texts = nullptr) {
  if (check_ctx(c)) return AMPH_E_PARAM;
  if (flags) return fail(AMPH_E_PARAM, "the gathered batch calls take host memory only (flags must be 0)");
  if (K == 0) return AMPH_OK;
  if (int st = check_parties(odos, n)) return st;
  if (!words || !first_fail || !bad_char || (!masked && !out16) || (masked && !secrets))
    return fail(AMPH_E_PARAM, "null pointer array or verdict array");
  const bool framed = out_texts != nullptr;
  std::vector<uint64_t> woff(K + 1, 0), toff(K, 0);
  size_t chars = 0;
  for (size_t o = 0; o < K; ++o) {
    const size_t nc = amph::wire_text_chars(words[o]);
    for (int j = 0; j < n; ++j) {
      const amph_odo_b64& t = odos[o * (size_t)n + j];
      if (t.nchars != nc)
        return fail(AMPH_E_LEN, "object " + std::to_string(o) + ", party " + std::to_string(j) +
                                    ": base64 fields of " + std::to_string(t.nchars) + " characters, expected " +
                                    std::to_string(nc) + " for " + std::to_string(words[o]) + " words");
      for (int k = 0; k < 5 && words[o]; ++k)
        if (!b64_field(t, k)) return fail(AMPH_E_PARAM, "object " + std::to_string(o) + ": null ODO field text");
    }
    if ((framed && !out_texts[o]) ||
        (words[o] && ((out16 && !out16[o]) || (out24 && !out24[o]) || (masked && !secrets[o]))))
      return fail(AMPH_E_PARAM, "object " + std::to_string(o) + ": null secrets/output");
    woff[o + 1] = woff[o] + words[o];
    toff[o] = chars;
    chars += amph::wire_slot_chars(words[o]);
  }
  WirePieces io;
  io.text = [&](int j, int k, size_t o) { return b64_field(odos[o * (size_t)n + j], k); };
  io.secrets = [&](size_t o) { return secrets[o]; };
  io.out16 = [&](size_t o) { return out16[o]; };
  io.out24 = [&](size_t o) { return out24[o]; };
  io.out_text = [&](size_t o) { return out_texts[o]; };
  return wire_batch_host(c, n, K, woff.data(), toff.data(), chars, masked, out16 != nullptr, out24 != nullptr, io,
                         first_fail, bad_char, framed);
}
}  // namespace

extern "C" {

size_t amph_wire_slot_chars(size_t words) { return amph::wire_slot_chars(words); }

uint64_t amph_wire_batch_copies(const amph_ctx* c) {
  return c ? first_device(c)->wire_copies.load(std::memory_order_relaxed) : 0;
}

int amph_recombine_verify_b64_packed(amph_ctx* c, const amph_odo_b64* odos, int n, const uint64_t* word_offsets,
                                     const uint64_t* text_offsets, size_t n_objects, uint8_t* out_secrets,
                                     int64_t* first_fail, int64_t* bad_char, uint32_t flags, void* stream) {
  return wire_packed_call(c, odos, n, word_offsets, text_offsets, n_objects, false, nullptr, out_secrets, nullptr,
                          first_fail, bad_char, flags, stream);
}

int amph_mask_input_b64_packed(amph_ctx* c, const amph_odo_b64* odos, int n, const uint64_t* word_offsets,
                               const uint64_t* text_offsets, size_t n_objects, const uint8_t* secrets,
                               uint8_t* out_masked16, char* out_records24, int64_t* first_fail, int64_t* bad_char,
                               uint32_t flags, void* stream) {
  return wire_packed_call(c, odos, n, word_offsets, text_offsets, n_objects, true, secrets, out_masked16,
                          out_records24, first_fail, bad_char, flags, stream);
}

int amph_recombine_verify_b64_batch(amph_ctx* c, const amph_odo_b64* odos, int n, size_t n_objects,
                                    const size_t* words, uint8_t* const* out_secrets, int64_t* first_fail,
                                    int64_t* bad_char, uint32_t flags) {
  return wire_batch_call(c, odos, n, n_objects, words, false, nullptr, out_secrets, nullptr, first_fail, bad_char,
                         flags);
}

int amph_mask_input_b64_batch(amph_ctx* c, const amph_odo_b64* odos, int n, size_t n_objects, const size_t* words,
                              const uint8_t* const* secrets, uint8_t* const* out_masked16,
                              char* const* out_records24, int64_t* first_fail, int64_t* bad_char, uint32_t flags) {
  return wire_batch_call(c, odos, n, n_objects, words, true, secrets, out_masked16, out_records24, first_fail,
                         bad_char, flags);
}

}  // extern "C"

// ---- many MaskedInput uploads per call (include/amphora_upload_batch.h) ---------
// Party side: K "data" array texts through k_conv_json_seg.  The image:
// [word table | text table | texts | tuples] in, [shares | K verdict words]
// out.  Client side: wire_batch_host's framed form (k_mask_json_seg).
namespace {
struct UploadPieces {  // object o's text, tuples and share rows
  std::function<const char*(size_t)> text;
  std::function<const uint8_t*(size_t)> tuples;
  std::function<uint8_t*(size_t)> out;
};

// woff validated; itoff[o] = where object o's text goes in the image's text
// region of `chars` bytes
int upload_conv_host(amph_ctx* c, size_t K, const uint64_t* woff, const std::vector<uint64_t>& itoff, size_t chars,
                     const UploadPieces& io, const W4& alpha, int use_zero, int64_t* bad_index) {
  const size_t T = woff[K];
  for (size_t o = 0; o < K; ++o) bad_index[o] = -1;
  BatchImage m;
  const size_t tab_w = m.in(8 * (K + 1)), tab_t = m.in(8 * K), txt = m.in(chars + 16), tup = m.in(32 * T + 16);
  const size_t osh = m.out(32 * T + 16);
  m.verdicts(K, "verdict array");
  if (int st = m.open(c, &amph_ctx::upload_copies, "upload")) return st;
  std::memcpy(m.host(tab_w), woff, 8 * (K + 1));
  std::memcpy(m.host(tab_t), itoff.data(), 8 * K);
  for (size_t o = 0; o < K; ++o) {
    const size_t w = woff[o + 1] - woff[o];
    std::memcpy(m.host(txt + itoff[o]), io.text(o), amph::masked_input_data_chars(w));
    if (w) std::memcpy(m.host(tup + 32 * woff[o]), io.tuples(o), 32 * w);
  }
  if (int st = m.upload()) return st;
  hipError_t e = amph::launch_convert_share_json_seg(
      (const char*)m.dev(txt), m.dev_table(tab_w), m.dev_table(tab_t), K,
      amph::wire_tile_grid(T, K, amph::kConvTileWords), (const uint4*)m.dev(tup), alpha, use_zero,
      (uint4*)m.dev(osh), m.dverd, m.c->f, cfg(m.c, m.s, T));
  if (int st = m.finish(e, "k_conv_json_seg")) return st;
  const unsigned long long* v = m.verdict_words();
  size_t nbad = 0, fb = 0;
  for (size_t o = 0; o < K; ++o) {
    const size_t w = woff[o + 1] - woff[o];
    if (v[o] != amph::kNoFail) {
      bad_index[o] = (int64_t)v[o];
      if (!nbad++) fb = o;
    }
    if (w) std::memcpy(io.out(o), m.host(osh + 32 * woff[o]), 32 * w);
  }
  if (nbad) {
    const int64_t bad = bad_index[fb];
    const std::string where = bad == 0 ? "the leading '['" : "record " + std::to_string((bad - 1) / 37);
    return fail(AMPH_E_PARAM, "object " + std::to_string(fb) + ": Malformed MaskedInput data text at offset " +
                                  std::to_string(bad) + " (" + where + "; " + std::to_string(nbad) + " of " +
                                  std::to_string(K) + " texts refused)");
  }
  return AMPH_OK;
}
}  // namespace

extern "C" {

size_t amph_upload_slot_chars(size_t words) { return amph::upload_slot_chars(words); }

uint64_t amph_upload_batch_copies(const amph_ctx* c) {
  return c ? first_device(c)->upload_copies.load(std::memory_order_relaxed) : 0;
}

int amph_convert_share_json_packed(amph_ctx* c, const char* texts, size_t texts_len, const uint64_t* woff,
                                   const uint64_t* toff, size_t K, const uint8_t* tuples,
                                   const uint8_t mac_key_le[16], int use_zero, uint8_t* out, int64_t* bad_index,
                                   uint32_t flags, void* stream) {
  if (check_ctx(c)) return AMPH_E_PARAM;
  AMPH_NO_HOST_IO(flags);
  if (K == 0) return AMPH_OK;
  if (!mac_key_le) return fail(AMPH_E_PARAM, "null mac key");
  if (!texts || !woff || !toff || !bad_index) return fail(AMPH_E_PARAM, "null text, offsets table or verdict array");
  const W4 alpha = amph::mont_mul(w4_of(ld128(mac_key_le)), amph::r2_word(c->f), c->f);
  if (flags & AMPH_F_DEVICE) {  // the texts at any byte alignment
    if (int st = check_dev_words({tuples, out})) return st;
    if (int st = tables_misaligned({woff, toff, bad_index})) return st;
    c = first_device(c);
    HIP_TRY(use_device(c->device));
    hipStream_t s = (hipStream_t)stream;
    if (int st = reset_verdicts_dev({bad_index}, K, flags, s)) return st;
    // the word table is the device's: every record takes 37 characters of the
    // texts, so T <= texts_len / 37 bounds the grid (surplus workgroups exit)
    const size_t tbound = texts_len / 37 + 1;
    hipError_t e = amph::launch_convert_share_json_seg(
        texts, woff, toff, K, amph::wire_tile_grid(tbound, K, amph::kConvTileWords), (const uint4*)tuples, alpha,
        use_zero, (uint4*)out, (unsigned long long*)bad_index, c->f, cfg(c, s, tbound));
    return e == hipSuccess ? AMPH_OK : hip_fail(e, "k_conv_json_seg");
  }
  if (int st = check_word_table(woff, K)) return st;
  if (int st = check_texts(kUploadTexts, woff, toff, K, texts_len)) return st;
  std::vector<uint64_t> itoff(K);
  size_t chars = 0;
  for (size_t o = 0; o < K; ++o) {
    chars += (toff[o] - chars) & 15;  // the image keeps every text's alignment
    itoff[o] = chars;
    chars += amph::masked_input_data_chars(woff[o + 1] - woff[o]);
  }
  if (woff[K] && (!tuples || !out)) return fail(AMPH_E_PARAM, "null tuples/output");
  UploadPieces io;
  io.text = [&](size_t o) { return texts + toff[o]; };
  io.tuples = [&](size_t o) { return tuples + 32 * woff[o]; };
  io.out = [&](size_t o) { return out + 32 * woff[o]; };
  return upload_conv_host(c, K, woff, itoff, chars, io, alpha, use_zero, bad_index);
}

int amph_convert_share_json_batch(amph_ctx* c, const char* const* texts, const size_t* lens, const size_t* words,
                                  size_t K, const uint8_t* const* tuples, const uint8_t mac_key_le[16],
                                  int use_zero, uint8_t* const* out, int64_t* bad_index, uint32_t flags) {
  if (check_ctx(c)) return AMPH_E_PARAM;
  if (flags) return fail(AMPH_E_PARAM, "the gathered batch calls take host memory only (flags must be 0)");
  if (K == 0) return AMPH_OK;
  if (!mac_key_le) return fail(AMPH_E_PARAM, "null mac key");
  if (!texts || !lens || !words || !tuples || !out || !bad_index)
    return fail(AMPH_E_PARAM, "null pointer array or verdict array");
  std::vector<uint64_t> woff(K + 1, 0), itoff(K);
  size_t chars = 0;
  for (size_t o = 0; o < K; ++o) {
    const size_t nc = amph::masked_input_data_chars(words[o]);
    if (lens[o] != nc)
      return fail(AMPH_E_LEN, "object " + std::to_string(o) + ": data array text of " + std::to_string(lens[o]) +
                                  " characters, expected " + std::to_string(nc) + " for " +
                                  std::to_string(words[o]) + " compact records");
    if (!texts[o] || (words[o] && (!tuples[o] || !out[o])))
      return fail(AMPH_E_PARAM, "object " + std::to_string(o) + ": null buffer");
    woff[o + 1] = woff[o] + words[o];
    itoff[o] = chars;  // the dense concatenation
    chars += nc;
  }
  const W4 alpha = amph::mont_mul(w4_of(ld128(mac_key_le)), amph::r2_word(c->f), c->f);
  UploadPieces io;
  io.text = [&](size_t o) { return texts[o]; };
  io.tuples = [&](size_t o) { return tuples[o]; };
  io.out = [&](size_t o) { return out[o]; };
  return upload_conv_host(c, K, woff.data(), itoff, chars, io, alpha, use_zero, bad_index);
}

int amph_mask_input_json_packed(amph_ctx* c, const amph_odo_b64* odos, int n, const uint64_t* woff,
                                const uint64_t* toff, size_t K, const uint8_t* secrets, char* out_text,
                                size_t out_cap, const uint64_t* ooff, int64_t* first_fail, int64_t* bad_char,
                                uint32_t flags, void* stream) {
  const FramedOut fr{ooff, out_text, out_cap};
  return wire_packed_call(c, odos, n, woff, toff, K, true, secrets, nullptr, nullptr, first_fail, bad_char, flags,
                          stream, &fr);
}

int amph_mask_input_json_batch(amph_ctx* c, const amph_odo_b64* odos, int n, size_t K, const size_t* words,
                               const uint8_t* const* secrets, char* const* out_texts, int64_t* first_fail,
                               int64_t* bad_char, uint32_t flags) {
  if (check_ctx(c)) return AMPH_E_PARAM;
  if (K && !flags && !out_texts) return fail(AMPH_E_PARAM, "null output text array");
  return wire_batch_call(c, odos, n, K, words, true, secrets, nullptr, nullptr, first_fail, bad_char, flags,
                         out_texts);
}

}  // extern "C"

// ---- many Output Delivery responses per call (include/amphora_respond_batch.h) ----
// The producer of the slotted field buffers the wire batch calls read: K
// objects' five packed word arrays through k_odo_b64_seg (codec.hip,
// respondtiles.hpp).  The image: [word table | text table | reject | 5 word
// arrays] in, the five field buffers up to the last text's end out --
// scattered text by text, so the caller's gaps stay untouched.  No verdicts:
// nothing to take back.
namespace {
const uint8_t* odo_words(const amph_odo& o, int k) {
  const uint8_t* const f[5] = {o.secret_shares, o.r_shares, o.v_shares, o.w_shares, o.u_shares};
  return f[k];
}
char* out_field(const amph_odo_b64_out& o, int k) {
  char* const f[5] = {o.secret_shares, o.r_shares, o.v_shares, o.w_shares, o.u_shares};
  return f[k];
}

// The host tables against T words and nchars characters: the wire batch
// calls' rules, and then the kernel's own geometry -- no object's range is
// clamped and no tile's text is clipped.
int check_respond_tables(const uint64_t* woff, const uint64_t* toff, size_t K, uint64_t T, size_t nchars) {
  if (int st = check_wire_tables(woff, toff, K, nchars)) return st;
  if (woff[K] != T)
    return fail(AMPH_E_PARAM, "word_offsets[" + std::to_string(K) + "] = " + std::to_string(woff[K]) +
                                  " differs from the fields' " + std::to_string(T) + " words");
  if (T > amph::kRespondMaxWords) return fail(AMPH_E_PARAM, "too many words for one call");
  for (size_t o = 0; o < K; ++o) {
    uint64_t w0, W;
    amph::respond_object_words(woff, o, T, &w0, &W);
    bool ok = w0 == woff[o] && W == woff[o + 1] - woff[o];
    if (ok && W) {
      const size_t last = (size_t)((W - 1) / amph::kWireTileWords);
      const amph::RespondTile t = amph::respond_tile(woff, toff, o, last, T, nchars);
      ok = t.words && t.store == t.chars && t.out_char == toff[o] + amph::kRespondTileChars * last &&
           t.out_char + t.chars == toff[o] + amph::wire_text_chars(W);
    }
    if (!ok) return fail(AMPH_E_PARAM, "object " + std::to_string(o) + ": its tiles leave the arrays or the buffers");
  }
  return AMPH_OK;
}

struct RespondPieces {  // object o's words of field k, and where its text of field k goes
  std::function<const uint8_t*(int, size_t)> in;
  std::function<char*(int, size_t)> out;
};

// tables validated, T = woff[K] > 0; `used` = the last text's end
int respond_host(amph_ctx* c, size_t K, const uint64_t* woff, const uint64_t* toff, size_t used,
                 const RespondPieces& io, const int64_t* reject) {
  const size_t T = woff[K], fchars = align256(used), fbytes = align256(16 * T);
  BatchImage m;
  const size_t tab_w = m.in(8 * (K + 1)), tab_t = m.in(8 * K), rej = m.in(reject ? 8 * K : 0);
  const size_t wrd = m.in(5 * fbytes), txt = m.out(5 * fchars);
  if (int st = m.open(c, &amph_ctx::respond_copies, "respond")) return st;
  std::memcpy(m.host(tab_w), woff, 8 * (K + 1));
  std::memcpy(m.host(tab_t), toff, 8 * K);
  if (reject) {  // the device's convention: kNoFail = clean
    unsigned long long* r = (unsigned long long*)m.host(rej);
    for (size_t o = 0; o < K; ++o) r[o] = reject[o] >= 0 ? (unsigned long long)reject[o] : amph::kNoFail;
  }
  const uint8_t* din[5];
  char* dout[5];
  for (int k = 0; k < 5; ++k) {
    for (size_t o = 0; o < K; ++o)
      if (const size_t w = woff[o + 1] - woff[o])
        std::memcpy(m.host(wrd + k * fbytes + 16 * woff[o]), io.in(k, o), 16 * w);
    din[k] = m.dev(wrd + k * fbytes);
    dout[k] = (char*)m.dev(txt + k * fchars);
  }
  if (int st = m.upload()) return st;
  hipError_t e = amph::launch_odo_b64_seg(din, dout, m.dev_table(tab_w), m.dev_table(tab_t), K,
                                          amph::wire_tile_grid(T, K), T, used,
                                          reject ? (const unsigned long long*)m.dev(rej) : nullptr,
                                          cfg(m.c, m.s, T));
  if (int st = m.finish(e, "k_odo_b64_seg")) return st;
  for (int k = 0; k < 5; ++k)
    for (size_t o = 0; o < K; ++o)
      if (const size_t nc = amph::wire_text_chars(woff[o + 1] - woff[o]))
        std::memcpy(io.out(k, o), m.host(txt + k * fchars + toff[o]), nc);
  return AMPH_OK;
}
}  // namespace

extern "C" {

uint64_t amph_respond_batch_copies(const amph_ctx* c) {
  return c ? first_device(c)->respond_copies.load(std::memory_order_relaxed) : 0;
}

int amph_odo_fields_b64_packed(amph_ctx* c, const amph_odo* fields, const uint64_t* woff, const uint64_t* toff,
                               size_t K, const amph_odo_b64_out* out, const int64_t* reject, uint32_t flags,
                               void* stream) {
  if (check_ctx(c)) return AMPH_E_PARAM;
  AMPH_NO_HOST_IO(flags);
  if (flags & AMPH_F_ACCUMULATE) return fail(AMPH_E_PARAM, "AMPH_F_ACCUMULATE is not accepted by this call");
  if (K == 0) return AMPH_OK;
  if (!fields || !out || !woff || !toff) return fail(AMPH_E_PARAM, "null fields, output or offsets table");
  if (fields->nbytes % 16) return fail(AMPH_E_LEN, "ODO field length must be a multiple of 16 bytes");
  const size_t T = fields->nbytes / 16;
  if (T == 0) return AMPH_OK;
  for (int k = 0; k < 5; ++k)
    if (!odo_words(*fields, k) || !out_field(*out, k)) return fail(AMPH_E_PARAM, "null ODO field or output text");
  if (flags & AMPH_F_DEVICE) {
    for (int k = 0; k < 5; ++k)
      if (int st = check_dev_words({odo_words(*fields, k), out_field(*out, k)})) return st;
    if (int st = tables_misaligned({woff, toff, reject})) return st;
    c = first_device(c);
    HIP_TRY(use_device(c->device));
    const uint8_t* din[5];
    char* dout[5];
    for (int k = 0; k < 5; ++k) {
      din[k] = odo_words(*fields, k);
      dout[k] = out_field(*out, k);
    }
    hipError_t e = amph::launch_odo_b64_seg(din, dout, woff, toff, K, amph::wire_tile_grid(T, K), T, out->nchars,
                                            (const unsigned long long*)reject, cfg(c, (hipStream_t)stream, T));
    return e == hipSuccess ? AMPH_OK : hip_fail(e, "k_odo_b64_seg");
  }
  if (int st = check_respond_tables(woff, toff, K, T, out->nchars)) return st;
  RespondPieces io;
  io.in = [&](int k, size_t o) { return odo_words(*fields, k) + 16 * woff[o]; };
  io.out = [&](int k, size_t o) { return out_field(*out, k) + toff[o]; };
  const size_t used = toff[K - 1] + amph::wire_text_chars(woff[K] - woff[K - 1]);  // the last text's end
  return respond_host(c, K, woff, toff, used, io, reject);
}

int amph_odo_fields_b64_batch(amph_ctx* c, const amph_odo* odos, size_t K, char* const* out_fields,
                              const int64_t* reject, uint32_t flags) {
  if (check_ctx(c)) return AMPH_E_PARAM;
  if (flags) return fail(AMPH_E_PARAM, "the gathered batch calls take host memory only (flags must be 0)");
  if (K == 0) return AMPH_OK;
  if (!odos || !out_fields) return fail(AMPH_E_PARAM, "null ODO array or output text array");
  std::vector<uint64_t> woff(K + 1, 0), toff(K, 0);
  size_t chars = 0, used = 0;
  for (size_t o = 0; o < K; ++o) {
    if (odos[o].nbytes % 16)
      return fail(AMPH_E_LEN, "object " + std::to_string(o) + ": ODO fields of " + std::to_string(odos[o].nbytes) +
                                  " bytes, not a multiple of 16");
    const size_t w = odos[o].nbytes / 16;
    for (int k = 0; k < 5 && w; ++k)
      if (!odo_words(odos[o], k) || !out_fields[5 * o + k])
        return fail(AMPH_E_PARAM, "object " + std::to_string(o) + ": null ODO field or output text");
    woff[o + 1] = woff[o] + w;
    toff[o] = chars;
    if (w) used = chars + amph::wire_text_chars(w);
    chars += amph::wire_slot_chars(w);
  }
  if (woff[K] == 0) return AMPH_OK;
  if (woff[K] > amph::kRespondMaxWords) return fail(AMPH_E_PARAM, "too many words for one call");
  RespondPieces io;
  io.in = [&](int k, size_t o) { return odo_words(odos[o], k); };
  io.out = [&](int k, size_t o) { return out_fields[5 * o + k]; };
  return respond_host(c, K, woff.data(), toff.data(), used, io, reject);
}

}  // extern "C"

// ---- many requests' Beaver exchange texts per call (include/amphora_exchange_batch.h) ----
// K objects' FactorPair array texts through the segmented codec (exchange.hip,
// exchangetiles.hpp).  Encode image: [pair table | text table | magnitudes |
// signs] in, [texts in dense slots | lengths] out.  Decode image: [pair table |
// text table | lengths | texts in dense slots] in, [magnitudes | signs | K
// verdict words] out.  The image's own slots are the dense layout whatever
// the caller's are: texts are gathered and scattered one by one, so the
// caller's gaps are neither read nor written.  The scans' scratch is
// c->xstage, device memory in either image mode.
namespace {
int check_pair_table(const uint64_t* poff, size_t K, size_t npairs) {
  if (poff[0] != 0) return fail(AMPH_E_PARAM, "pair_offsets[0] must be 0");
  for (size_t o = 0; o < K; ++o)
    if (poff[o + 1] < poff[o])
      return fail(AMPH_E_PARAM, "pair_offsets must not decrease (entry " + std::to_string(o + 1) + ")");
  if (poff[K] != npairs)
    return fail(AMPH_E_PARAM, "pair_offsets[" + std::to_string(K) + "] = " + std::to_string(poff[K]) +
                                  " differs from npairs_total = " + std::to_string(npairs));
  if (npairs > ((size_t)1 << 48)) return fail(AMPH_E_PARAM, "too many pairs for one call");
  return AMPH_OK;
}

// object o's `chars(o)` characters at toff[o] (a multiple of the span) end
// before the next slot, which starts later, and before the capacity
int check_exchange_slots(const uint64_t* toff, size_t K, const std::function<uint64_t(size_t)>& chars, uint64_t cap,
                         const char* cap_name) {
  for (size_t o = 0; o < K; ++o) {
    const uint64_t end = toff[o] + chars(o);
    const bool next = o + 1 < K;
    if (toff[o] % AMPH_EXCHANGE_SLOT_ALIGN)
      return fail(AMPH_E_PARAM, "text_offsets[" + std::to_string(o) + "] = " + std::to_string(toff[o]) +
                                    " must be a multiple of " + std::to_string(AMPH_EXCHANGE_SLOT_ALIGN));
    if (end < toff[o] || end > (next ? toff[o + 1] : cap) || (next && toff[o + 1] <= toff[o]))
      return fail(AMPH_E_PARAM, "object " + std::to_string(o) + ": its text [" + std::to_string(toff[o]) + ", " +
                                    std::to_string(end) + ") runs past " +
                                    (next ? "the next slot at " + std::to_string(toff[o + 1])
                                          : std::string(cap_name) + " = " + std::to_string(cap)));
  }
  return AMPH_OK;
}

int exchange_scratch(amph_ctx* c, size_t bytes, void** p) {
  if (dev_ensure(c, c->xstage, bytes) != hipSuccess) return fail(AMPH_E_NOMEM, "exchange scratch");
  *p = c->xstage.p;
  return AMPH_OK;
}

struct XEncPieces {  // object o's diffs, and its text's destination with its capacity
  std::function<const uint8_t*(size_t)> mag, neg;
  std::function<char*(size_t)> out;
  std::function<size_t(size_t)> cap;
};

// poff validated (poff[K] = T pairs)
int exchange_encode_host(amph_ctx* c, size_t K, const uint64_t* poff, const XEncPieces& io, uint64_t* out_lens) {
  const size_t T = poff[K];
  std::vector<uint64_t> itoff(K);
  size_t chars = 0;
  for (size_t o = 0; o < K; ++o) {
    itoff[o] = chars;
    chars += amph::xseg_slot_chars(poff[o + 1] - poff[o]);
  }
  BatchImage m;
  const size_t tab_p = m.in(8 * (K + 1)), tab_t = m.in(8 * K), mg = m.in(32 * T + 16), ng = m.in(2 * T + 16);
  const size_t txt = m.out(chars), lens = m.out(8 * K);
  if (int st = m.open(c, &amph_ctx::exchange_copies, "exchange")) return st;
  void* scratch;
  if (int st = exchange_scratch(m.c, amph::xencs_scratch_bytes(T, K), &scratch)) return st;
  std::memcpy(m.host(tab_p), poff, 8 * (K + 1));
  std::memcpy(m.host(tab_t), itoff.data(), 8 * K);
  for (size_t o = 0; o < K; ++o)
    if (const size_t P = poff[o + 1] - poff[o]) {
      std::memcpy(m.host(mg + 32 * poff[o]), io.mag(o), 32 * P);
      std::memcpy(m.host(ng + 2 * poff[o]), io.neg(o), 2 * P);
    }
  if (int st = m.upload()) return st;
  hipError_t e = amph::launch_exchange_encode_seg((const uint4*)m.dev(mg), m.dev(ng), T, m.dev_table(tab_p),
                                                  m.dev_table(tab_t), K, (char*)m.dev(txt), chars,
                                                  (unsigned long long*)m.dev(lens), scratch, cfg(m.c, m.s, T));
  if (int st = m.finish(e, "k_xencs")) return st;
  const uint64_t* got = (const uint64_t*)m.host(lens);
  size_t nshort = 0, first = 0;
  for (size_t o = 0; o < K; ++o) {
    out_lens[o] = got[o];
    if (got[o] > io.cap(o)) {
      if (!nshort++) first = o;
      continue;
    }
    std::memcpy(io.out(o), m.host(txt + itoff[o]), got[o]);
  }
  if (nshort)
    return fail(AMPH_E_LEN, "object " + std::to_string(first) + ": output capacity " + std::to_string(io.cap(first)) +
                                " below the encoded length " + std::to_string(got[first]) + " (" +
                                std::to_string(nshort) + " of " + std::to_string(K) + " texts do not fit)");
  return AMPH_OK;
}

struct XDecPieces {  // object o's text, and where its diffs go
  std::function<const char*(size_t)> text;
  std::function<uint8_t*(size_t)> mag, neg;
};

// poff validated; len[o] = object o's characters
int exchange_decode_host(amph_ctx* c, size_t K, const uint64_t* poff, const std::function<size_t(size_t)>& len,
                         const XDecPieces& io, int64_t* bad_index) {
  const size_t T = poff[K];
  std::vector<uint64_t> itoff(K), ilen(K);
  size_t chars = 0;
  for (size_t o = 0; o < K; ++o) {
    itoff[o] = chars;
    ilen[o] = len(o);
    const size_t slot = (ilen[o] + AMPH_EXCHANGE_SLOT_ALIGN - 1) & ~(size_t)(AMPH_EXCHANGE_SLOT_ALIGN - 1);
    chars += slot ? slot : AMPH_EXCHANGE_SLOT_ALIGN;
    bad_index[o] = -1;
  }
  BatchImage m;
  const size_t tab_p = m.in(8 * (K + 1)), tab_t = m.in(8 * K), tab_l = m.in(8 * K), txt = m.in(chars);
  const size_t mg = m.out(32 * T + 16), ng = m.out(2 * T + 16);
  m.verdicts(K, "verdict array");
  if (int st = m.open(c, &amph_ctx::exchange_copies, "exchange")) return st;
  void* scratch;
  if (int st = exchange_scratch(m.c, amph::xdecs_scratch_bytes(chars, K), &scratch)) return st;
  std::memcpy(m.host(tab_p), poff, 8 * (K + 1));
  std::memcpy(m.host(tab_t), itoff.data(), 8 * K);
  std::memcpy(m.host(tab_l), ilen.data(), 8 * K);
  for (size_t o = 0; o < K; ++o)
    if (ilen[o]) std::memcpy(m.host(txt + itoff[o]), io.text(o), ilen[o]);
  if (int st = m.upload()) return st;  // (resets the verdict words)
  hipError_t e = amph::launch_exchange_decode_seg((const char*)m.dev(txt), chars, m.dev_table(tab_p),
                                                  m.dev_table(tab_t), m.dev_table(tab_l), K, T, (uint4*)m.dev(mg),
                                                  m.dev(ng), m.dverd, false, scratch, cfg(m.c, m.s, chars));
  if (int st = m.finish(e, "k_xdecs")) return st;
  const unsigned long long* v = m.verdict_words();
  size_t nbad = 0, nlen = 0, fb = 0, fl = 0;
  for (size_t o = 0; o < K; ++o) {
    const size_t P = poff[o + 1] - poff[o];
    if (v[o] == amph::kNoFail) {
      if (P) {
        std::memcpy(io.mag(o), m.host(mg + 32 * poff[o]), 32 * P);
        std::memcpy(io.neg(o), m.host(ng + 2 * poff[o]), 2 * P);
      }
      continue;
    }
    bad_index[o] = (int64_t)v[o];
    if (v[o] == ilen[o]) {
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
                                std::to_string(poff[fl + 1] - poff[fl]) + " FactorPairs (" + std::to_string(nlen) +
                                " of " + std::to_string(K) + " texts refused)");
  return AMPH_OK;
}

const char* const kGatherHostOnly = "the gathered batch calls take host memory only (flags must be 0)";
}  // namespace

extern "C" {

size_t amph_exchange_slot_chars(size_t npairs) { return amph::xseg_slot_chars(npairs); }

uint64_t amph_exchange_batch_copies(const amph_ctx* c) {
  return c ? first_device(c)->exchange_copies.load(std::memory_order_relaxed) : 0;
}

int amph_exchange_encode_packed(amph_ctx* c, const uint8_t* mag16, const uint8_t* neg, size_t npairs,
                                const uint64_t* poff, const uint64_t* toff, size_t K, char* out, size_t out_cap,
                                uint64_t* out_lens, uint32_t flags, void* stream) {
  if (check_ctx(c)) return AMPH_E_PARAM;
  AMPH_NO_HOST_IO(flags);
  if (flags & AMPH_F_ACCUMULATE) return fail(AMPH_E_PARAM, "AMPH_F_ACCUMULATE is not accepted by this call");
  if (K == 0) return AMPH_OK;
  if (!poff || !toff || !out || !out_lens || (npairs && (!mag16 || !neg)))
    return fail(AMPH_E_PARAM, "null diffs, offsets table, output text or length array");
  if (flags & AMPH_F_DEVICE) {
    if (int st = check_dev_words({mag16, out})) return st;
    if (int st = tables_misaligned({poff, toff, out_lens})) return st;
    c = first_device(c);
    HIP_TRY(use_device(c->device));
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> g(c->mu);
    void* scratch;
    if (int st = dev_scratch(c, amph::xencs_scratch_bytes(npairs, K), s, &scratch)) return st;
    hipError_t e = amph::launch_exchange_encode_seg((const uint4*)mag16, neg, npairs, poff, toff, K, out, out_cap,
                                                    (unsigned long long*)out_lens, scratch, cfg(c, s, npairs));
    if (e != hipSuccess) return hip_fail(e, "k_xencs");
    HIP_TRY(hipEventRecord(c->xdev_done, s));
    return AMPH_OK;
  }
  if (int st = check_pair_table(poff, K, npairs)) return st;
  if (int st = check_exchange_slots(
          toff, K, [&](size_t o) { return (uint64_t)amph::xseg_max_chars(poff[o + 1] - poff[o]); }, out_cap,
          "out_cap"))
    return st;
  XEncPieces io;
  io.mag = [&](size_t o) { return mag16 + 32 * poff[o]; };
  io.neg = [&](size_t o) { return neg + 2 * poff[o]; };
  io.out = [&](size_t o) { return out + toff[o]; };
  io.cap = [&](size_t o) { return amph::xseg_max_chars(poff[o + 1] - poff[o]); };
  return exchange_encode_host(c, K, poff, io, out_lens);
}

int amph_exchange_encode_batch(amph_ctx* c, const uint8_t* const* mag16, const uint8_t* const* neg,
                               const size_t* npairs, size_t K, char* const* out, const size_t* out_caps,
                               uint64_t* out_lens, uint32_t flags) {
  if (check_ctx(c)) return AMPH_E_PARAM;
  if (flags) return fail(AMPH_E_PARAM, kGatherHostOnly);
  if (K == 0) return AMPH_OK;
  if (!mag16 || !neg || !npairs || !out || !out_caps || !out_lens)
    return fail(AMPH_E_PARAM, "null pointer array, capacity array or length array");
  std::vector<uint64_t> poff(K + 1, 0);
  for (size_t o = 0; o < K; ++o) {
    if (!out[o] || (npairs[o] && (!mag16[o] || !neg[o])))
      return fail(AMPH_E_PARAM, "object " + std::to_string(o) + ": null buffer");
    poff[o + 1] = poff[o] + npairs[o];
  }
  if (int st = check_pair_table(poff.data(), K, poff[K])) return st;
  XEncPieces io;
  io.mag = [&](size_t o) { return mag16[o]; };
  io.neg = [&](size_t o) { return neg[o]; };
  io.out = [&](size_t o) { return out[o]; };
  io.cap = [&](size_t o) { return out_caps[o]; };
  return exchange_encode_host(c, K, poff.data(), io, out_lens);
}

int amph_exchange_decode_packed(amph_ctx* c, const char* texts, size_t texts_len, const uint64_t* poff,
                                const uint64_t* toff, const uint64_t* tlen, size_t K, size_t npairs,
                                uint8_t* mag16, uint8_t* neg, int64_t* bad_index, uint32_t flags, void* stream) {
  if (check_ctx(c)) return AMPH_E_PARAM;
  AMPH_NO_HOST_IO(flags);
  if (K == 0) return AMPH_OK;
  if (!poff || !toff || !tlen || !bad_index || (texts_len && !texts) || (npairs && (!mag16 || !neg)))
    return fail(AMPH_E_PARAM, "null texts, offsets table, diffs or verdict array");
  if (flags & AMPH_F_DEVICE) {
    if (int st = check_dev_words({mag16, texts})) return st;
    if (int st = tables_misaligned({poff, toff, tlen, bad_index})) return st;
    c = first_device(c);
    HIP_TRY(use_device(c->device));
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> g(c->mu);
    void* scratch;
    if (int st = dev_scratch(c, amph::xdecs_scratch_bytes(texts_len, K), s, &scratch)) return st;
    hipError_t e = amph::launch_exchange_decode_seg(texts, texts_len, poff, toff, tlen, K, npairs, (uint4*)mag16, neg,
                                                    (unsigned long long*)bad_index, !(flags & AMPH_F_ACCUMULATE),
                                                    scratch, cfg(c, s, texts_len));
    if (e != hipSuccess) return hip_fail(e, "k_xdecs");
    HIP_TRY(hipEventRecord(c->xdev_done, s));
    return AMPH_OK;
  }
  if (flags & AMPH_F_ACCUMULATE) return fail(AMPH_E_PARAM, "AMPH_F_ACCUMULATE needs AMPH_F_DEVICE here");
  if (int st = check_pair_table(poff, K, npairs)) return st;
  if (int st = check_exchange_slots(toff, K, [&](size_t o) { return tlen[o]; }, texts_len, "texts_len")) return st;
  XDecPieces io;
  io.text = [&](size_t o) { return texts + toff[o]; };
  io.mag = [&](size_t o) { return mag16 + 32 * poff[o]; };
  io.neg = [&](size_t o) { return neg + 2 * poff[o]; };
  return exchange_decode_host(c, K, poff, [&](size_t o) { return (size_t)tlen[o]; }, io, bad_index);
}

int amph_exchange_decode_batch(amph_ctx* c, const char* const* texts, const size_t* lens, const size_t* npairs,
                               size_t K, uint8_t* const* mag16, uint8_t* const* neg, int64_t* bad_index,
                               uint32_t flags) {
  if (check_ctx(c)) return AMPH_E_PARAM;
  if (flags) return fail(AMPH_E_PARAM, kGatherHostOnly);
  if (K == 0) return AMPH_OK;
  if (!texts || !lens || !npairs || !mag16 || !neg || !bad_index)
    return fail(AMPH_E_PARAM, "null pointer array or verdict array");
  std::vector<uint64_t> poff(K + 1, 0);
  for (size_t o = 0; o < K; ++o) {
    if ((lens[o] && !texts[o]) || (npairs[o] && (!mag16[o] || !neg[o])))
      return fail(AMPH_E_PARAM, "object " + std::to_string(o) + ": null buffer");
    poff[o + 1] = poff[o] + npairs[o];
  }
  if (int st = check_pair_table(poff.data(), K, poff[K])) return st;
  XDecPieces io;
  io.text = [&](size_t o) { return texts[o]; };
  io.mag = [&](size_t o) { return mag16[o]; };
  io.neg = [&](size_t o) { return neg[o]; };
  return exchange_decode_host(c, K, poff.data(), [&](size_t o) { return lens[o]; }, io, bad_index);
}

}  // extern "C"
