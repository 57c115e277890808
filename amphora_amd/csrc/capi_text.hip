// C ABI of libamphora_hip (declared in include/amphora.h): the text forms --
// base64, the Beaver open exchange codec, K_RV / K_MASK from the wire texts
// and K_CONV from the MaskedInput "data" array text.
#include "capi_internal.hpp"
#include "wiretiles.hpp"
#include "respondtiles.hpp"

// ---- base64 wire codec ---------------------------------------------------------
namespace {
size_t b64_padding(const char* last2) {
  return (last2[1] == '=') + (last2[1] == '=' && last2[0] == '=');
}

// Host-path helper for the < 1-unit tail: copy in, run, copy out, synchronously.
template <class Launch>
int run_tail(amph_ctx* c, const void* in, size_t in_bytes, void* out, size_t out_bytes,
             bool with_bad, unsigned long long* bad_host, Launch&& launch) {
  HIP_TRY(use_device(c->device));
  hipError_t e = dev_ensure(c, c->tail, 512);
  if (e != hipSuccess) return fail(AMPH_E_NOMEM, "tail scratch");
  if (!c->streams[0]) HIP_TRY(hipStreamCreateWithFlags(&c->streams[0], hipStreamNonBlocking));
  hipStream_t s = c->streams[0];  // the context's own stream: no device-wide sync
  uint8_t* d = (uint8_t*)c->tail.p;
  // `in` is caller memory, pageable in general: a blocking copy after the
  // stream is idle (kPageableRule, above read_back)
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipMemcpy(d, in, in_bytes, hipMemcpyHostToDevice));
  if (with_bad) HIP_TRY(hipMemsetAsync(d + 448, 0x7F, 8, s));
  e = launch(d, d + 256, (unsigned long long*)(d + 448), cfg(c, s, 1));
  if (e != hipSuccess) return hip_fail(e, "codec tail");
  HIP_TRY(read_back(s, {{out, d + 256, out_bytes}, {bad_host, d + 448, with_bad ? (size_t)8 : 0}}));
  return AMPH_OK;
}
}  // namespace
extern "C" {

int amph_base64_encode(amph_ctx* c, const uint8_t* in, size_t nbytes, char* out, uint32_t flags,
                       void* stream) {
  if (check_ctx(c)) return AMPH_E_PARAM;
  AMPH_NO_HOST_IO(flags);
  if (nbytes && (!in || !out)) return fail(AMPH_E_PARAM, "null buffer");
  if (flags & AMPH_F_DEVICE) {
    HIP_TRY(use_device(c->device));
    hipError_t e = amph::launch_b64_encode(in, nbytes, out, cfg(c, (hipStream_t)stream, (nbytes + 11) / 12));
    return e == hipSuccess ? AMPH_OK : hip_fail(e, "k_b64_encode");
  }
  std::lock_guard<std::mutex> g(c->mu);
  const size_t units = nbytes / 12, rem = nbytes % 12;
  int st = run_batched(c, units, {arr_in(in, 12)}, {arr_out(out, 16)}, false, nullptr,
                       [&](auto& din, auto& dout, size_t cnt, unsigned long long*,
                           const amph::LaunchCfg& lc) {
                         return amph::launch_b64_encode((const uint8_t*)din[0], 12 * cnt,
                                                        (char*)dout[0], lc);
                       });
  if (st != AMPH_OK || rem == 0) return st;
  return run_tail(c, in + 12 * units, rem, out + 16 * units, 4 * ((rem + 2) / 3), false, nullptr,
                  [&](uint8_t* di, uint8_t* dout, unsigned long long*, const amph::LaunchCfg& lc) {
                    return amph::launch_b64_encode(di, rem, (char*)dout, lc);
                  });
}

int amph_base64_decode(amph_ctx* c, const char* in, size_t nchars, uint8_t* out,
                       size_t* out_bytes, int64_t* bad_index, uint32_t flags, void* stream) {
  if (check_ctx(c)) return AMPH_E_PARAM;
  AMPH_NO_HOST_IO(flags);
  if (nchars % 4) return fail(AMPH_E_LEN, "base64 input length must be a multiple of 4");
  if (nchars && (!in || !out)) return fail(AMPH_E_PARAM, "null buffer");
  if (bad_index && !(flags & AMPH_F_DEVICE)) *bad_index = -1;
  if (nchars == 0) {
    if (out_bytes) *out_bytes = 0;
    return AMPH_OK;
  }
  char last2[2];
  if (flags & AMPH_F_DEVICE) {
    HIP_TRY(use_device(c->device));
    if (!bad_index) return fail(AMPH_E_PARAM, "bad_index is required");
    // out_bytes given: one 2-byte read-back decides the padding (the only
    // synchronous step); null: fully asynchronous, the kernel sizes it
    size_t ob = amph::kB64PadOnDevice;
    if (out_bytes) {
      HIP_TRY(read_back((hipStream_t)stream, {{last2, in + nchars - 2, 2}}));
      ob = 3 * nchars / 4 - b64_padding(last2);
      *out_bytes = ob;
    }
    if (int st = reset_ff_dev(bad_index, flags, (hipStream_t)stream)) return st;
    hipError_t e = amph::launch_b64_decode(in, nchars, out, ob, (unsigned long long*)bad_index,
                                           cfg(c, (hipStream_t)stream, (nchars + 15) / 16));
    return e == hipSuccess ? AMPH_OK : hip_fail(e, "k_b64_decode");
  }
  std::lock_guard<std::mutex> g(c->mu);
  std::memcpy(last2, in + nchars - 2, 2);
  const size_t ob = 3 * nchars / 4 - b64_padding(last2);
  if (out_bytes) *out_bytes = ob;
  // full 16-char units that contain no padding go through the batched path
  const size_t units = (nchars - 4) / 16, tail_chars = nchars - 16 * units;
  int64_t bad = -1;
  int st = run_batched(c, units, {arr_in(in, 16)}, {arr_out(out, 12)}, true, &bad,
                       [&](auto& din, auto& dout, size_t cnt, unsigned long long* ff,
                           const amph::LaunchCfg& lc) {
                         return amph::launch_b64_decode((const char*)din[0], 16 * cnt,
                                                        (uint8_t*)dout[0], 12 * cnt, ff, lc,
                                                        false);  // batches never end the text
                       },
                       16);  // the kernel reports a character offset, 16 per unit
  if (st != AMPH_OK && st != AMPH_E_VERIFY) return st;
  unsigned long long tb = amph::kNoFail;
  const size_t tail_out = ob - 12 * units;
  int st2 = run_tail(c, in + 16 * units, tail_chars, out + 12 * units, tail_out, true, &tb,
                     [&](uint8_t* di, uint8_t* dout, unsigned long long* bb, const amph::LaunchCfg& lc) {
                       return amph::launch_b64_decode((const char*)di, tail_chars, dout, tail_out,
                                                      bb, lc);
                     });
  if (st2 != AMPH_OK) return st2;
  // the tail kernel saw the tail as the whole text, so its '=' rule is exact
  const int64_t first = st == AMPH_E_VERIFY ? bad : (tb != amph::kNoFail ? (int64_t)(16 * units + tb) : -1);
  if (first >= 0) {
    if (bad_index) *bad_index = first;
    return fail(AMPH_E_PARAM, "Illegal base64 character at index " + std::to_string(first));
  }
  return AMPH_OK;
}

int amph_base64_encode_words(amph_ctx* c, const uint8_t* words16, size_t words, char* out24,
                             uint32_t flags, void* stream) {
  if (check_ctx(c)) return AMPH_E_PARAM;
  AMPH_NO_HOST_IO(flags);
  if (words && (!words16 || !out24)) return fail(AMPH_E_PARAM, "null buffer");
  return run_words(c, words, {arr_in(words16, 16), arr_out(out24, 24, 8)}, false, nullptr, flags, stream,
                   "k_b64_words",
                   [&](const DevIn& din, const DevOut& dout, size_t cnt, unsigned long long*,
                       const amph::LaunchCfg& lc) {
                     return amph::launch_b64_words(din[0], cnt, (char*)dout[0], lc);
                   });
}

int amph_base64_decode_words(amph_ctx* c, const char* in24, size_t words, uint8_t* out16,
                             int64_t* bad_index, uint32_t flags, void* stream) {
  if (check_ctx(c)) return AMPH_E_PARAM;
  AMPH_NO_HOST_IO(flags);
  if (words && (!in24 || !out16)) return fail(AMPH_E_PARAM, "null buffer");
  // device mode reports into the caller's word; host mode turns the index into a message
  const bool dev = flags & AMPH_F_DEVICE;
  int64_t bad = -1;
  int st = run_words(c, words, {arr_out(out16, 16), arr_in(in24, 24, 8)}, true, dev ? bad_index : &bad, flags,
                     stream, "k_b64_unwords",
                     [&](const DevIn& din, const DevOut& dout, size_t cnt, unsigned long long* ff,
                         const amph::LaunchCfg& lc) {
                       return amph::launch_b64_unwords((const char*)din[0], cnt, dout[0], ff, lc);
                     });
  if (dev) return st;
  if (bad_index) *bad_index = bad;
  if (st == AMPH_E_VERIFY)
    return fail(AMPH_E_PARAM, "Illegal base64 word record at index " + std::to_string(bad));
  return st;
}

}  // extern "C"

namespace capi __attribute__((visibility("hidden"))) {
// the verdict word of an exchange decode (`pairs` FactorPairs expected in
// `len` characters) as the call's status and message
int decode_status(int64_t bad, size_t len, size_t pairs, int64_t* bad_index) {
  if (bad == (int64_t)AMPH_NO_FAILURE) return AMPH_OK;
  if (bad_index) *bad_index = bad;
  if ((size_t)bad == len)
    return fail(AMPH_E_LEN, "interimValues must hold exactly " + std::to_string(pairs) + " FactorPairs");
  return fail(AMPH_E_PARAM, "Malformed FactorPair JSON at offset " + std::to_string(bad));
}
}  // namespace capi

extern "C" {

// ---- Beaver open exchange codec ------------------------------------------------
namespace {
// Host-pointer calls of the exchange codec: one shot on the context's first
// stream (the whole text is scanned at once, so there is no batching).
//
// Device-pointer calls take their scan scratch from one per-context buffer:
// under the context mutex each call makes its stream wait for the previous
// call's kernels (xdev_done) before reusing it, then records its own.  (The
// device's stream-ordered pool handed two contexts overlapping buffers in
// the host paths)
int dev_scratch(amph_ctx* c, size_t bytes, hipStream_t s, void** p) {
  if (!c->xdev_done) HIP_TRY(hipEventCreateWithFlags(&c->xdev_done, hipEventDisableTiming));
  else HIP_TRY(hipStreamWaitEvent(s, c->xdev_done, 0));
  if (c->xdev.cap < bytes) {
    HIP_TRY(hipEventSynchronize(c->xdev_done));  // the old buffer is idle before it is freed
    if (dev_ensure(c, c->xdev, bytes) != hipSuccess) return fail(AMPH_E_NOMEM, "exchange scratch");
  }
  *p = c->xdev.p;
  return AMPH_OK;
}
}  // namespace

size_t amph_exchange_max_chars(size_t npairs) { return amph::xenc_max_bytes(npairs); }

int amph_exchange_encode(amph_ctx* c, const uint8_t* mag16, const uint8_t* neg, size_t npairs,
                         char* out, size_t out_cap, uint64_t* out_len, uint32_t flags,
                         void* stream) {
  if (check_ctx(c)) return AMPH_E_PARAM;
  AMPH_NO_HOST_IO(flags);
  if (!out || !out_len || (npairs && (!mag16 || !neg))) return fail(AMPH_E_PARAM, "null buffer");
  HIP_TRY(use_device(c->device));
  const size_t maxb = amph::xenc_max_bytes(npairs);
  if (flags & AMPH_F_DEVICE) {
    if (int st = check_dev_words({mag16})) return st;
    if (out_cap < maxb) return fail(AMPH_E_LEN, "output capacity below amph_exchange_max_chars(npairs)");
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> g(c->mu);
    void* scratch;
    if (int st = dev_scratch(c, amph::xenc_scratch_bytes(npairs), s, &scratch)) return st;
    hipError_t e = amph::launch_exchange_encode((const uint4*)mag16, neg, npairs, out,
                                                (unsigned long long*)out_len, scratch, cfg(c, s, npairs));
    if (e != hipSuccess) return hip_fail(e, "k_xenc");
    HIP_TRY(hipEventRecord(c->xdev_done, s));
    return AMPH_OK;
  }
  // host mode: diffs in, text and its length out.  A small call's kernel
  // writes the length straight into the arena head: one synchronisation and
  // no verdict-copy kernel.
  std::lock_guard<std::mutex> g(c->mu);
  const size_t arena = align256(32 * npairs) + align256(2 * npairs) + align256(maxb);
  const size_t sb = amph::xenc_scratch_bytes(npairs);
  const bool small = npairs && small_call(c, arena);
  hipStream_t s;
  if (int st = host_stream(c, small ? 1 : 0, &s)) return st;
  Stager h;
  if (int st = h.begin(c, s, small, arena, 0, &c->xstage,
                       small ? carve_bytes({sb}) : carve_bytes({32 * npairs, 2 * npairs, maxb, 8, sb}),
                       "exchange staging"))
    return st;
  uint8_t *dmag = h.take(32 * npairs), *dneg = h.take(2 * npairs), *dtext = h.take(maxb);
  unsigned long long* dlen = h.result_word();
  if (npairs) {
    HIP_TRY(h.put(dmag, mag16, 32 * npairs));
    HIP_TRY(h.put(dneg, neg, 2 * npairs));
  }
  hipError_t e = amph::launch_exchange_encode((const uint4*)dmag, dneg, npairs, (char*)dtext, dlen,
                                              h.scratch(sb), cfg(c, s, npairs));
  if (e != hipSuccess) return h.launch_failed(e, "k_xenc");
  uint64_t len = 0;
  if (int st = h.finish(nullptr, {{&len, dlen, 8}})) return st;
  *out_len = len;
  if (len > out_cap) return fail(AMPH_E_LEN, "output capacity " + std::to_string(out_cap) +
                                                 " below the encoded length " + std::to_string(len));
  return h.fetch({{out, dtext, len}});
}

int amph_exchange_decode(amph_ctx* c, const char* text, size_t len, size_t npairs, uint8_t* mag16,
                         uint8_t* neg, int64_t* bad_index, uint32_t flags, void* stream) {
  if (check_ctx(c)) return AMPH_E_PARAM;
  AMPH_NO_HOST_IO(flags);
  if ((len && !text) || (npairs && (!mag16 || !neg))) return fail(AMPH_E_PARAM, "null buffer");
  HIP_TRY(use_device(c->device));
  if (flags & AMPH_F_DEVICE) {
    if (int st = check_dev_words({mag16})) return st;
    hipStream_t s = (hipStream_t)stream;
    if (int st = reset_ff_dev(bad_index, flags, s)) return st;
    std::lock_guard<std::mutex> g(c->mu);
    void* scratch;
    if (int st = dev_scratch(c, amph::xdec_scratch_bytes(len), s, &scratch)) return st;
    hipError_t e = amph::launch_exchange_decode(text, len, npairs, (uint4*)mag16, neg,
                                                (unsigned long long*)bad_index, scratch, cfg(c, s, len));
    if (e != hipSuccess) return hip_fail(e, "k_xdec");
    HIP_TRY(hipEventRecord(c->xdev_done, s));
    return AMPH_OK;
  }
  std::lock_guard<std::mutex> g(c->mu);
  // host mode: text in, diffs out (copied only from a well-formed text)
  const size_t arena = align256(len) + align256(32 * npairs) + align256(2 * npairs);
  const size_t sb = amph::xdec_scratch_bytes(len);
  const bool small = len && small_call(c, arena);
  hipStream_t s;
  if (int st = host_stream(c, small ? 1 : 0, &s)) return st;
  Stager h;
  if (int st = h.begin(c, s, small, arena, 1, &c->xstage,
                       small ? carve_bytes({sb}) : carve_bytes({len, 32 * npairs, 2 * npairs, 8, sb}),
                       "exchange staging"))
    return st;
  uint8_t *dtext = h.take(len), *dmag = h.take(32 * npairs), *dneg = h.take(2 * npairs);
  if (len) HIP_TRY(h.put(dtext, text, len));
  if (int st = h.arm()) return st;
  hipError_t e = amph::launch_exchange_decode((const char*)dtext, len, npairs, (uint4*)dmag, dneg, h.fl,
                                              h.scratch(sb), cfg(c, s, len));
  if (e != hipSuccess) return h.launch_failed(e, "k_xdec");
  int64_t bad = 0;
  if (int st = h.finish(&bad, {})) return st;
  if (bad_index) *bad_index = -1;
  if (int st = decode_status(bad, len, npairs, bad_index)) return st;
  return h.fetch({{mag16, dmag, 32 * npairs}, {neg, dneg, 2 * npairs}});
}

// ---- K_RV / K_MASK from the wire ----------------------------------------------
namespace {
const char* const kOdoFieldNames[5] = {"secretShares", "rShares", "vShares", "wShares", "uShares"};

const char* b64_field(const amph_odo_b64& o, int k) {
  switch (k) {
    case 0: return o.secret_shares;
    case 1: return o.r_shares;
    case 2: return o.v_shares;
    case 3: return o.w_shares;
    default: return o.u_shares;
  }
}

// Shared checks; *nchars / *pad for `words` 16-byte words.
int wire_check(const amph_odo_b64* odos, int n, size_t words, size_t* nchars, uint32_t* pad) {
  if (!odos || n < 1 || n > AMPH_MAX_PARTIES)
    return fail(AMPH_E_PARAM, "n_parties must be in [1, 16] with a non-null ODO array");
  const size_t nb = 16 * words;
  *nchars = 4 * ((nb + 2) / 3);
  *pad = (uint32_t)((3 - nb % 3) % 3);
  for (int j = 0; j < n; ++j) {
    if (odos[j].nchars != *nchars)
      return fail(AMPH_E_LEN, "party " + std::to_string(j) + ": base64 fields of " +
                                  std::to_string(odos[j].nchars) + " characters, expected " +
                                  std::to_string(*nchars) + " for " + std::to_string(words) + " words");
    for (int k = 0; k < 5 && words; ++k)
      if (!b64_field(odos[j], k)) return fail(AMPH_E_PARAM, "null ODO field text");
  }
  return AMPH_OK;
}

int wire_bad_message(int64_t bad, size_t nchars) {
  const size_t o = (size_t)bad / nchars, at = (size_t)bad % nchars;
  return fail(AMPH_E_PARAM, "Illegal base64 character at index " + std::to_string(at) + " of party " +
                                std::to_string(o / 5) + "'s " + kOdoFieldNames[o % 5]);
}

// Host mode of the wire-text calls: one launch on the context's first stream
// over the Stager's buffers -- the 5 n field texts (the kernels' TextSet),
// `extra` bytes of further inputs and outputs, and two verdict words
// (first-fail, bad character).
static int wire_stage(amph_ctx* c, const amph_odo_b64* odos, int n, size_t nchars, size_t extra, hipStream_t s,
               Stager* h, amph::TextSet* tx) {
  const size_t bytes = 5 * n * align256(nchars ? nchars : 16) + extra + 256;
  const bool small = small_call(c, bytes);
  if (int st = h->begin(c, s, small, bytes, 2, &c->wire, small ? 0 : bytes, "wire staging")) return st;
  for (int j = 0; j < n; ++j)
    for (int k = 0; k < 5; ++k) {
      uint8_t* d = h->take(nchars);
      if (nchars) HIP_TRY(h->put(d, b64_field(odos[j], k), nchars));
      tx->t[k][j] = (const char*)d;
    }
  return h->arm();
}

// what the two verdict words of a wire-text call say
static int wire_status(const int64_t v[2], size_t nchars, int64_t* first_fail, int64_t* bad_char) {
  if (v[1] != (int64_t)AMPH_NO_FAILURE) {
    if (bad_char) *bad_char = v[1];
    return wire_bad_message(v[1], nchars);
  }
  if (v[0] != (int64_t)AMPH_NO_FAILURE) {
    if (first_fail) *first_fail = v[0];
    return AMPH_E_VERIFY;
  }
  return AMPH_OK;
}
}  // namespace

int amph_recombine_verify_b64(amph_ctx* c, const amph_odo_b64* odos, int n, size_t words,
                              uint8_t* out_secrets, int64_t* first_fail, int64_t* bad_char,
                              uint32_t flags, void* stream) {
  if (check_ctx(c)) return AMPH_E_PARAM;
  AMPH_NO_HOST_IO(flags);
  size_t nchars;
  uint32_t pad;
  if (int st = wire_check(odos, n, words, &nchars, &pad)) return st;
  if (words && !out_secrets) return fail(AMPH_E_PARAM, "null output");
  HIP_TRY(use_device(c->device));
  if (flags & AMPH_F_DEVICE) {
    amph::TextSet tx{};
    for (int j = 0; j < n; ++j)
      for (int k = 0; k < 5; ++k) {
        tx.t[k][j] = b64_field(odos[j], k);
        if (int st = check_dev_words({tx.t[k][j]})) return st;
      }
    if (int st = check_dev_words({out_secrets})) return st;
    hipStream_t s = (hipStream_t)stream;
    if (int st = reset_ff_dev(first_fail, flags, s)) return st;
    if (int st = reset_ff_dev(bad_char, flags, s)) return st;
    hipError_t e = amph::launch_rv_b64(tx, n, words, nchars, pad, (uint4*)out_secrets,
                                       (unsigned long long*)first_fail, (unsigned long long*)bad_char,
                                       c->f, cfg(c, s, words));
    return e == hipSuccess ? AMPH_OK : hip_fail(e, "k_rv_b64");
  }
  if (first_fail) *first_fail = -1;
  if (bad_char) *bad_char = -1;
  if (words == 0) return AMPH_OK;
  std::lock_guard<std::mutex> g(c->mu);
  hipStream_t s;
  if (int st = host_stream(c, 0, &s)) return st;
  Stager h;
  amph::TextSet tx{};
  if (int st = wire_stage(c, odos, n, nchars, align256(16 * words) + 256, s, &h, &tx)) return st;
  uint8_t* dout = h.take(16 * words);
  hipError_t e = amph::launch_rv_b64(tx, n, words, nchars, pad, (uint4*)dout, h.fl, h.fl + 1, c->f,
                                     cfg(c, s, words));
  if (e != hipSuccess) return h.launch_failed(e, "k_rv_b64");
  int64_t v[2];
  if (int st = h.finish(v, {{out_secrets, dout, 16 * words}})) return st;
  return wire_status(v, nchars, first_fail, bad_char);
}

size_t amph_masked_input_data_chars(size_t words) { return words ? 37 * words + 1 : 2; }

// amph_mask_input_b64 / amph_mask_input_json: out_text (the framed "data"
// array, amph_masked_input_data_chars(n_secrets) characters) excludes the
// other two outputs.
static int mask_input_wire(amph_ctx* c, const amph_odo_b64* odos, int n, size_t words,
                           const uint8_t* secrets, size_t n_secrets, uint8_t* out16, char* out24,
                           char* out_text, size_t out_cap, int64_t* first_fail, int64_t* bad_char,
                           uint32_t flags, void* stream) {
  if (check_ctx(c)) return AMPH_E_PARAM;
  AMPH_NO_HOST_IO(flags);
  size_t nchars;
  uint32_t pad;
  if (int st = wire_check(odos, n, words, &nchars, &pad)) return st;
  if (n_secrets > words) {
    // as amph_mask_input: the texts decode and every mask verifies before the
    // length error (DefaultAmphoraClient.java:153 before :160)
    int st = amph_mask_input_b64(c, odos, n, words, nullptr, 0, nullptr, nullptr, first_fail, bad_char,
                                 flags, stream);
    if (st != AMPH_OK) return st;
    if (flags & AMPH_F_DEVICE) {
      HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
      int64_t v[2] = {(int64_t)AMPH_NO_FAILURE, (int64_t)AMPH_NO_FAILURE};
      if (first_fail) HIP_TRY(hipMemcpy(&v[0], first_fail, 8, hipMemcpyDeviceToHost));  // kPageableRule
      if (bad_char) HIP_TRY(hipMemcpy(&v[1], bad_char, 8, hipMemcpyDeviceToHost));
      if (v[1] != (int64_t)AMPH_NO_FAILURE) return wire_bad_message(v[1], nchars);
      if (v[0] != (int64_t)AMPH_NO_FAILURE)
        return fail(AMPH_E_VERIFY, "input mask MAC check failed at word " + std::to_string(v[0]));
    }
    return fail(AMPH_E_LEN, "more secret words than verified input masks");
  }
  if (n_secrets && !secrets) return fail(AMPH_E_PARAM, "null secrets");
  const size_t text_chars = amph_masked_input_data_chars(n_secrets);
  if (out_text && out_cap < text_chars)
    return fail(AMPH_E_LEN, "output capacity " + std::to_string(out_cap) + " below the " +
                                std::to_string(text_chars) + " characters of " + std::to_string(n_secrets) +
                                " records");
  HIP_TRY(use_device(c->device));
  if (flags & AMPH_F_DEVICE) {
    amph::TextSet tx{};
    for (int j = 0; j < n; ++j)
      for (int k = 0; k < 5; ++k) {
        tx.t[k][j] = b64_field(odos[j], k);
        if (int st = check_dev_words({tx.t[k][j]})) return st;
      }
    if (int st = check_dev_words({secrets, out16, out24, out_text})) return st;
    hipStream_t s = (hipStream_t)stream;
    if (int st = reset_ff_dev(first_fail, flags, s)) return st;
    if (int st = reset_ff_dev(bad_char, flags, s)) return st;
    if (out_text && n_secrets) {
      hipError_t e = amph::launch_mask_json(tx, n, words, nchars, pad, (const uint4*)secrets, n_secrets, out_text,
                                            (unsigned long long*)first_fail, (unsigned long long*)bad_char,
                                            c->f, cfg(c, s, words));
      return e == hipSuccess ? AMPH_OK : hip_fail(e, "k_mask_json");
    }
    if (out_text) {  // no secrets: "[]", and the masks are still verified
      HIP_TRY(hipMemsetAsync(out_text, '[', 1, s));
      HIP_TRY(hipMemsetAsync(out_text + 1, ']', 1, s));
    }
    hipError_t e = amph::launch_mask_b64(tx, n, words, nchars, pad, (const uint4*)secrets, n_secrets,
                                         (uint4*)out16, out24, (unsigned long long*)first_fail,
                                         (unsigned long long*)bad_char, c->f, cfg(c, s, words));
    return e == hipSuccess ? AMPH_OK : hip_fail(e, "k_mask_b64");
  }
  if (first_fail) *first_fail = -1;
  if (bad_char) *bad_char = -1;
  if (out_text && n_secrets == 0) {
    out_text[0] = '[';
    out_text[1] = ']';
    out_text = nullptr;
  }
  if (words == 0) return AMPH_OK;
  std::lock_guard<std::mutex> g(c->mu);
  hipStream_t s;
  if (int st = host_stream(c, 0, &s)) return st;
  Stager h;
  amph::TextSet tx{};
  const size_t extra = 3 * align256(16 * n_secrets) + align256(24 * n_secrets) +
                       (out_text ? align256(text_chars) : 0) + 1024;
  if (int st = wire_stage(c, odos, n, nchars, extra, s, &h, &tx)) return st;
  uint8_t* dsec = h.take(16 * n_secrets);
  uint8_t* d16 = h.take(16 * n_secrets);
  uint8_t* d24 = h.take(24 * n_secrets);
  uint8_t* dtext = out_text ? h.take(text_chars) : nullptr;
  if (n_secrets) HIP_TRY(h.put(dsec, secrets, 16 * n_secrets));
  hipError_t e = out_text ? amph::launch_mask_json(tx, n, words, nchars, pad, (const uint4*)dsec, n_secrets,
                                                   (char*)dtext, h.fl, h.fl + 1, c->f, cfg(c, s, words))
                          : amph::launch_mask_b64(tx, n, words, nchars, pad, (const uint4*)dsec, n_secrets,
                                                  out16 ? (uint4*)d16 : nullptr, out24 ? (char*)d24 : nullptr,
                                                  h.fl, h.fl + 1, c->f, cfg(c, s, words));
  if (e != hipSuccess) return h.launch_failed(e, out_text ? "k_mask_json" : "k_mask_b64");
  int64_t v[2];
  if (int st = h.finish(v, {{out16, d16, out16 ? 16 * n_secrets : 0},
                            {out24, d24, out24 ? 24 * n_secrets : 0},
                            {out_text, dtext, out_text ? text_chars : 0}}))
    return st;
  return wire_status(v, nchars, first_fail, bad_char);
}

int amph_mask_input_b64(amph_ctx* c, const amph_odo_b64* odos, int n, size_t words,
                        const uint8_t* secrets, size_t n_secrets, uint8_t* out16, char* out24,
                        int64_t* first_fail, int64_t* bad_char, uint32_t flags, void* stream) {
  return mask_input_wire(c, odos, n, words, secrets, n_secrets, out16, out24, nullptr, 0, first_fail, bad_char,
                         flags, stream);
}

int amph_mask_input_json(amph_ctx* c, const amph_odo_b64* odos, int n, size_t words,
                         const uint8_t* secrets, size_t n_secrets, char* out_text, size_t out_cap,
                         int64_t* first_fail, int64_t* bad_char, uint32_t flags, void* stream) {
  if (check_ctx(c)) return AMPH_E_PARAM;
  if (!out_text && n_secrets <= words) return fail(AMPH_E_PARAM, "null output text");
  return mask_input_wire(c, odos, n, words, secrets, n_secrets, nullptr, nullptr, out_text, out_cap, first_fail,
                         bad_char, flags, stream);
}

// ---- K_CONV from the MaskedInput "data" array text -------------------------------
int amph_convert_share_json(amph_ctx* c, const char* text, size_t len, size_t words,
                            const uint8_t* tuples, const uint8_t mac_key_le[16], int use_zero,
                            uint8_t* out, int64_t* bad_index, uint32_t flags, void* stream) {
  if (check_ctx(c)) return AMPH_E_PARAM;
  AMPH_NO_HOST_IO(flags);
  if (!mac_key_le) return fail(AMPH_E_PARAM, "null mac key");
  if (len != amph_masked_input_data_chars(words))
    return fail(AMPH_E_LEN, "data array text of " + std::to_string(len) + " characters, expected " +
                                std::to_string(amph_masked_input_data_chars(words)) + " for " +
                                std::to_string(words) + " compact records");
  if (!text || (words && (!tuples || !out))) return fail(AMPH_E_PARAM, "null buffer");
  const W4 alpha = amph::mont_mul(w4_of(ld128(mac_key_le)), amph::r2_word(c->f), c->f);
  HIP_TRY(use_device(c->device));
  if (flags & AMPH_F_DEVICE) {  // the text at any byte alignment
    if (int st = check_dev_words({tuples, out})) return st;
    hipStream_t s = (hipStream_t)stream;
    if (int st = reset_ff_dev(bad_index, flags, s)) return st;
    hipError_t e = amph::launch_convert_share_json(text, (const uint4*)tuples, words, alpha, use_zero, (uint4*)out,
                                                   (unsigned long long*)bad_index, c->f, cfg(c, s, words));
    return e == hipSuccess ? AMPH_OK : hip_fail(e, "k_conv_json");
  }
  // host mode: one shot on the context's first stream, in the exchange
  // codec's staging buffer; never through the small-call arena
  if (bad_index) *bad_index = -1;
  std::lock_guard<std::mutex> g(c->mu);
  hipStream_t s;
  if (int st = host_stream(c, 0, &s)) return st;
  Stager h;
  if (int st = h.begin(c, s, false, 0, 1, &c->xstage, carve_bytes({len, 32 * words, 32 * words, 8}),
                       "exchange staging"))
    return st;
  uint8_t *dtext = h.take(len), *dtup = h.take(32 * words), *dout = h.take(32 * words);
  HIP_TRY(h.put(dtext, text, len));
  if (words) HIP_TRY(h.put(dtup, tuples, 32 * words));
  if (int st = h.arm()) return st;
  hipError_t e = amph::launch_convert_share_json((const char*)dtext, (const uint4*)dtup, words, alpha, use_zero,
                                                 (uint4*)dout, h.fl, c->f, cfg(c, s, words));
  if (e != hipSuccess) return h.launch_failed(e, "k_conv_json");
  int64_t bad = 0;
  if (int st = h.finish(&bad, {})) return st;
  if (bad != (int64_t)AMPH_NO_FAILURE) {
    if (bad_index) *bad_index = bad;
    const std::string where = bad == 0 ? "the leading '['" : "record " + std::to_string((bad - 1) / 37);
    return fail(AMPH_E_PARAM, "Malformed MaskedInput data text at offset " + std::to_string(bad) + " (" + where + ")");
  }
  return h.fetch({{out, dout, 32 * words}});
}

}  // extern "C"

// ---- K_RV / K_MASK from the wire, many objects per call -------------------------
// include/amphora_wire_batch.h: the slotted text layout (wire.hip,
// wiretiles.hpp).  Host mode moves ONE page-locked image to the device and one
// back, whatever the object count: [word table | text table | 5 n field
// buffers | secrets] in, [16-byte words | records | 2 K verdict words] out.
// A call that fits the small-call arena builds the image there and the
// kernel reads and writes it in place; its verdict arrays stay in device
// memory (atomics) and come to the arena by launch_take_array before the
// call's one synchronisation, as run_packed_small.
namespace {
int wire_batch_parties(const amph_odo_b64* odos, int n) {
  if (!odos || n < 1 || n > AMPH_MAX_PARTIES)
    return fail(AMPH_E_PARAM, "n_parties must be in [1, 16] with a non-null ODO array");
  return AMPH_OK;
}

// the host tables of a packed call against the buffers' length
int check_wire_tables(const uint64_t* woff, const uint64_t* toff, size_t K, size_t nchars) {
  if (woff[0] != 0) return fail(AMPH_E_PARAM, "word_offsets[0] must be 0");
  for (size_t o = 0; o < K; ++o)
    if (woff[o + 1] < woff[o])
      return fail(AMPH_E_PARAM, "word_offsets must not decrease (entry " + std::to_string(o + 1) + ")");
  for (size_t o = 0; o < K; ++o) {
    const uint64_t end = toff[o] + amph::wire_text_chars(woff[o + 1] - woff[o]);
    if (toff[o] % 16)
      return fail(AMPH_E_PARAM, "text_offsets[" + std::to_string(o) + "] = " + std::to_string(toff[o]) +
                                    " must be a multiple of 16");
    if (end < toff[o] || end > (o + 1 < K ? toff[o + 1] : (uint64_t)nchars))
      return fail(AMPH_E_PARAM, "object " + std::to_string(o) + ": its text [" + std::to_string(toff[o]) + ", " +
                                    std::to_string(end) + ") runs past " +
                                    (o + 1 < K ? "the next slot at " + std::to_string(toff[o + 1])
                                               : "the buffers' " + std::to_string(nchars) + " characters"));
  }
  return AMPH_OK;
}

// The verdict words (first-fail array, then bad-character array) as the
// caller's entries and the call's status.
int wire_batch_status(const unsigned long long* v, size_t K, const uint64_t* woff, int64_t* first_fail,
                      int64_t* bad_char) {
  size_t nbad = 0, nfail = 0, fb = 0, ff = 0;
  for (size_t o = 0; o < K; ++o) {
    const bool bad = v[K + o] != amph::kNoFail, failed = !bad && v[o] != amph::kNoFail;
    if (bad && !nbad++) fb = o;
    if (failed && !nfail++) ff = o;
    bad_char[o] = bad ? (int64_t)v[K + o] : -1;
    first_fail[o] = failed ? (int64_t)v[o] : -1;
  }
  if (nbad) {
    const size_t nc = amph::wire_text_chars(woff[fb + 1] - woff[fb]), f = (size_t)v[K + fb] / nc;
    return fail(AMPH_E_PARAM, "object " + std::to_string(fb) + ": Illegal base64 character at index " +
                                  std::to_string((size_t)v[K + fb] % nc) + " of party " + std::to_string(f / 5) +
                                  "'s " + kOdoFieldNames[f % 5] + " (" + std::to_string(nbad) + " of " +
                                  std::to_string(K) + " objects hold an illegal character)");
  }
  if (nfail)
    return fail(AMPH_E_VERIFY, "Verification of secret has failed: object " + std::to_string(ff) + " at word " +
                                   std::to_string(v[ff]) + " (" + std::to_string(nfail) + " of " +
                                   std::to_string(K) + " objects failed)");
  return AMPH_OK;
}

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
  if (!c->sub.empty()) c = c->sub[0];
  std::atomic<uint64_t>& copies = framed ? c->upload_copies : c->wire_copies;
  const char* kernel = framed ? "k_mask_json_seg" : masked ? "k_mask_b64_seg" : "k_rv_b64_seg";
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(use_device(c->device));
  hipStream_t s;
  if (int st = host_stream(c, 0, &s)) return st;
  const size_t fchars = align256(chars ? chars : 16);
  const size_t tab_w = 0, tab_t = tab_w + align256(8 * (K + 1)), tab_o = tab_t + align256(8 * K);
  const size_t txt = tab_o + (framed ? align256(8 * K) : 0);
  const size_t sec = txt + 5 * (size_t)n * fchars, in_bytes = sec + (masked ? align256(16 * T) : 0);
  const size_t o16 = in_bytes, o24 = o16 + (want16 ? align256(16 * T) : 0);
  const size_t otx = o24 + (want24 ? align256(24 * T) : 0);
  size_t ochars = 0;  // the framed texts' slots: object o's at the sum of its predecessors' strides
  for (size_t o = 0; framed && o < K; ++o) ochars += amph::upload_slot_chars(woff[o + 1] - woff[o]);
  const size_t verd = otx + align256(ochars), total = verd + align256(16 * K);
  const bool small = small_call(c, total);
  uint8_t *himg, *dimg;
  unsigned long long* dverd;
  if (small) {
    if (c->small.ensure(total + 256) != hipSuccess) return fail(AMPH_E_NOMEM, "small-call arena");
    if (dev_ensure(c, c->seg, 16 * K) != hipSuccess) return fail(AMPH_E_NOMEM, "verdict arrays");
    himg = dimg = (uint8_t*)c->small.p;
    dverd = (unsigned long long*)c->seg.p;
  } else {
    if (c->wire_img.ensure(total) != hipSuccess) return fail(AMPH_E_NOMEM, "wire batch image");
    if (dev_ensure(c, c->wire, total) != hipSuccess) return fail(AMPH_E_NOMEM, "wire staging");
    himg = (uint8_t*)c->wire_img.p;
    dimg = (uint8_t*)c->wire.p;
    dverd = (unsigned long long*)(dimg + verd);
  }
  std::memcpy(himg + tab_w, woff, 8 * (K + 1));
  std::memcpy(himg + tab_t, toff, 8 * K);
  uint64_t* ooff = (uint64_t*)(himg + tab_o);
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
          std::memcpy(himg + at + toff[o], io.text(j, k, o), nc);
      tx.t[k][j] = (const char*)(dimg + at);
    }
  for (size_t o = 0; masked && o < K; ++o)
    if (woff[o + 1] > woff[o]) std::memcpy(himg + sec + 16 * woff[o], io.secrets(o), 16 * (woff[o + 1] - woff[o]));
  if (!small) {  // page-locked image, idle stream: one blocking copy (kPageableRule)
    HIP_TRY(hipMemcpy(dimg, himg, in_bytes, hipMemcpyHostToDevice));
    copies.fetch_add(1, std::memory_order_relaxed);
  }
  HIP_TRY(hipMemsetAsync(dverd, 0x7F, 16 * K, s));
  const uint64_t *dw = (const uint64_t*)(dimg + tab_w), *dt = (const uint64_t*)(dimg + tab_t);
  const size_t grid = amph::wire_tile_grid(T, K);
  hipError_t e = framed ? amph::launch_mask_json_seg(tx, n, dw, dt, (const uint64_t*)(dimg + tab_o), K, grid,
                                                     (const uint4*)(dimg + sec), (char*)(dimg + otx), dverd,
                                                     dverd + K, c->f, cfg(c, s, T))
                 : masked ? amph::launch_mask_b64_seg(tx, n, dw, dt, K, grid, (const uint4*)(dimg + sec),
                                                    want16 ? (uint4*)(dimg + o16) : nullptr,
                                                    want24 ? (char*)(dimg + o24) : nullptr, dverd, dverd + K, c->f,
                                                    cfg(c, s, T))
                        : amph::launch_rv_b64_seg(tx, n, dw, dt, K, grid, (uint4*)(dimg + o16), dverd, dverd + K,
                                                  c->f, cfg(c, s, T));
  if (e == hipSuccess && small) e = amph::launch_take_array(dverd, (unsigned long long*)(himg + verd), 2 * K, s);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(s);
    return hip_fail(e, kernel);
  }
  HIP_TRY(hipStreamSynchronize(s));
  if (!small) {
    HIP_TRY(hipMemcpy(himg + in_bytes, dimg + in_bytes, total - in_bytes, hipMemcpyDeviceToHost));
    copies.fetch_add(1, std::memory_order_relaxed);
  }
  for (size_t o = 0; o < K; ++o) {
    const size_t w0 = woff[o], w = woff[o + 1] - w0;
    if (framed) std::memcpy(io.out_text(o), himg + otx + ooff[o], amph::masked_input_data_chars(w));
    if (!w) continue;
    if (want16) std::memcpy(io.out16(o), himg + o16 + 16 * w0, 16 * w);
    if (want24) std::memcpy(io.out24(o), himg + o24 + 24 * w0, 24 * w);
  }
  return wire_batch_status((const unsigned long long*)(himg + verd), K, woff, first_fail, bad_char);
}

// Both packed calls: `masked` = false runs K_RV (out16 = the secrets out).
int wire_packed_call(amph_ctx* c, const amph_odo_b64* odos, int n, const uint64_t* woff, const uint64_t* toff,
                     size_t K, bool masked, const uint8_t* secrets, uint8_t* out16, char* out24,
                     int64_t* first_fail, int64_t* bad_char, uint32_t flags, void* stream) {
  if (check_ctx(c)) return AMPH_E_PARAM;
  AMPH_NO_HOST_IO(flags);
  if (K == 0) return AMPH_OK;
  if (int st = wire_batch_parties(odos, n)) return st;
  if (!woff || !toff || !first_fail || !bad_char)
    return fail(AMPH_E_PARAM, "null offsets table or verdict array");
  for (int j = 1; j < n; ++j)
    if (odos[j].nchars != odos[0].nchars)
      return fail(AMPH_E_LEN, "party " + std::to_string(j) + ": field buffers of " + std::to_string(odos[j].nchars) +
                                  " characters, party 0's hold " + std::to_string(odos[0].nchars));
  const size_t nchars = odos[0].nchars;
  if (flags & AMPH_F_DEVICE) {
    amph::TextSet tx{};
    for (int j = 0; j < n; ++j)
      for (int k = 0; k < 5; ++k) {
        tx.t[k][j] = b64_field(odos[j], k);
        if (nchars && !tx.t[k][j]) return fail(AMPH_E_PARAM, "null ODO field text");
        if (int st = check_dev_words({tx.t[k][j]})) return st;
      }
    if (int st = check_dev_words({secrets, out16, out24})) return st;
    if (((uintptr_t)woff | (uintptr_t)toff | (uintptr_t)first_fail | (uintptr_t)bad_char) & 7)
      return fail(AMPH_E_PARAM, "device offset tables and verdict arrays must be 8-byte aligned");
    if (nchars && ((!masked && !out16) || (masked && !secrets))) return fail(AMPH_E_PARAM, "null secrets/output");
    if (!c->sub.empty()) c = c->sub[0];
    HIP_TRY(use_device(c->device));
    hipStream_t s = (hipStream_t)stream;
    if (!(flags & AMPH_F_ACCUMULATE)) {
      HIP_TRY(hipMemsetAsync(first_fail, 0x7F, 8 * K, s));
      HIP_TRY(hipMemsetAsync(bad_char, 0x7F, 8 * K, s));
    }
    // the word table is the device's: every text of W words takes at least
    // 64 W / 3 characters of the buffers, so T <= 3 nchars / 64 bounds the
    // grid (the surplus workgroups find no tile and exit)
    const size_t tbound = 3 * (nchars / 64) + 3, grid = amph::wire_tile_grid(tbound, K);
    if (nchars == 0) return AMPH_OK;
    hipError_t e = masked ? amph::launch_mask_b64_seg(tx, n, woff, toff, K, grid, (const uint4*)secrets,
                                                      (uint4*)out16, out24, (unsigned long long*)first_fail,
                                                      (unsigned long long*)bad_char, c->f, cfg(c, s, tbound))
                          : amph::launch_rv_b64_seg(tx, n, woff, toff, K, grid, (uint4*)out16,
                                                    (unsigned long long*)first_fail,
                                                    (unsigned long long*)bad_char, c->f, cfg(c, s, tbound));
    return e == hipSuccess ? AMPH_OK : hip_fail(e, masked ? "k_mask_b64_seg" : "k_rv_b64_seg");
  }
  if (int st = check_wire_tables(woff, toff, K, nchars)) return st;
  const size_t T = woff[K];
  if (T) {
    for (int j = 0; j < n; ++j)
      for (int k = 0; k < 5; ++k)
        if (!b64_field(odos[j], k)) return fail(AMPH_E_PARAM, "null ODO field text");
    if ((!masked && !out16) || (masked && !secrets)) return fail(AMPH_E_PARAM, "null secrets/output");
  }
  WirePieces io;
  io.text = [&](int j, int k, size_t o) { return b64_field(odos[j], k) + toff[o]; };
  io.secrets = [&](size_t o) { return secrets + 16 * woff[o]; };
  io.out16 = [&](size_t o) { return out16 + 16 * woff[o]; };
  io.out24 = [&](size_t o) { return out24 + 24 * woff[o]; };
  const size_t used = toff[K - 1] + amph::wire_text_chars(woff[K] - woff[K - 1]);  // the last text's end
  return wire_batch_host(c, n, K, woff, toff, used, masked, out16 != nullptr, out24 != nullptr, io, first_fail,
                         bad_char);
}

// The gathered calls: odos[o * n + j], one words[o] per object.  out_texts
// (amph_mask_input_json_batch): the framed texts instead of out16 / out24.
int wire_batch_call(amph_ctx* c, const amph_odo_b64* odos, int n, size_t K, const size_t* words, bool masked,
                    const uint8_t* const* secrets, uint8_t* const* out16, char* const* out24,
                    int64_t* first_fail, int64_t* bad_char, uint32_t flags, char* const* out_texts = nullptr) {
  if (check_ctx(c)) return AMPH_E_PARAM;
  if (flags) return fail(AMPH_E_PARAM, "the gathered batch calls take host memory only (flags must be 0)");
  if (K == 0) return AMPH_OK;
  if (int st = wire_batch_parties(odos, n)) return st;
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
  if (!c) return 0;
  return (c->sub.empty() ? c : c->sub[0])->wire_copies.load(std::memory_order_relaxed);
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
// Party side: K "data" array texts through k_conv_json_seg.  Host mode as the
// wire batch calls': ONE page-locked image in -- [word table | text table |
// texts | tuples] -- and one back -- [shares | K verdict words]; a call that
// fits the small-call arena is built there, with its verdict words in device
// memory (atomics) until launch_take_array brings them over.
// Client side: wire_batch_host's framed form (k_mask_json_seg).
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
  if (!c->sub.empty()) c = c->sub[0];
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(use_device(c->device));
  hipStream_t s;
  if (int st = host_stream(c, 0, &s)) return st;
  const size_t tab_w = 0, tab_t = tab_w + align256(8 * (K + 1)), txt = tab_t + align256(8 * K);
  const size_t tup = txt + align256(chars + 16), in_bytes = tup + align256(32 * T + 16);
  const size_t osh = in_bytes, verd = osh + align256(32 * T + 16), total = verd + align256(8 * K);
  const bool small = small_call(c, total);
  uint8_t *himg, *dimg;
  unsigned long long* dverd;
  if (small) {
    if (c->small.ensure(total + 256) != hipSuccess) return fail(AMPH_E_NOMEM, "small-call arena");
    if (dev_ensure(c, c->seg, 8 * K) != hipSuccess) return fail(AMPH_E_NOMEM, "verdict array");
    himg = dimg = (uint8_t*)c->small.p;
    dverd = (unsigned long long*)c->seg.p;
  } else {
    if (c->wire_img.ensure(total) != hipSuccess) return fail(AMPH_E_NOMEM, "upload batch image");
    if (dev_ensure(c, c->wire, total) != hipSuccess) return fail(AMPH_E_NOMEM, "upload staging");
    himg = (uint8_t*)c->wire_img.p;
    dimg = (uint8_t*)c->wire.p;
    dverd = (unsigned long long*)(dimg + verd);
  }
  std::memcpy(himg + tab_w, woff, 8 * (K + 1));
  std::memcpy(himg + tab_t, itoff.data(), 8 * K);
  for (size_t o = 0; o < K; ++o) {
    const size_t w = woff[o + 1] - woff[o];
    std::memcpy(himg + txt + itoff[o], io.text(o), amph::masked_input_data_chars(w));
    if (w) std::memcpy(himg + tup + 32 * woff[o], io.tuples(o), 32 * w);
  }
  if (!small) {  // page-locked image, idle stream: one blocking copy (kPageableRule)
    HIP_TRY(hipMemcpy(dimg, himg, in_bytes, hipMemcpyHostToDevice));
    c->upload_copies.fetch_add(1, std::memory_order_relaxed);
  }
  HIP_TRY(hipMemsetAsync(dverd, 0x7F, 8 * K, s));
  hipError_t e = amph::launch_convert_share_json_seg(
      (const char*)(dimg + txt), (const uint64_t*)(dimg + tab_w), (const uint64_t*)(dimg + tab_t), K,
      amph::wire_tile_grid(T, K, amph::kConvTileWords), (const uint4*)(dimg + tup), alpha, use_zero,
      (uint4*)(dimg + osh), dverd, c->f, cfg(c, s, T));
  if (e == hipSuccess && small) e = amph::launch_take_array(dverd, (unsigned long long*)(himg + verd), K, s);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(s);
    return hip_fail(e, "k_conv_json_seg");
  }
  HIP_TRY(hipStreamSynchronize(s));
  if (!small) {
    HIP_TRY(hipMemcpy(himg + in_bytes, dimg + in_bytes, total - in_bytes, hipMemcpyDeviceToHost));
    c->upload_copies.fetch_add(1, std::memory_order_relaxed);
  }
  const unsigned long long* v = (const unsigned long long*)(himg + verd);
  size_t nbad = 0, fb = 0;
  for (size_t o = 0; o < K; ++o) {
    const size_t w = woff[o + 1] - woff[o];
    if (v[o] != amph::kNoFail) {
      bad_index[o] = (int64_t)v[o];
      if (!nbad++) fb = o;
    }
    if (w) std::memcpy(io.out(o), himg + osh + 32 * woff[o], 32 * w);
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

int check_word_table(const uint64_t* woff, size_t K) {
  if (woff[0] != 0) return fail(AMPH_E_PARAM, "word_offsets[0] must be 0");
  for (size_t o = 0; o < K; ++o)
    if (woff[o + 1] < woff[o])
      return fail(AMPH_E_PARAM, "word_offsets must not decrease (entry " + std::to_string(o + 1) + ")");
  return AMPH_OK;
}
}  // namespace

extern "C" {

size_t amph_upload_slot_chars(size_t words) { return amph::upload_slot_chars(words); }

uint64_t amph_upload_batch_copies(const amph_ctx* c) {
  if (!c) return 0;
  return (c->sub.empty() ? c : c->sub[0])->upload_copies.load(std::memory_order_relaxed);
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
    if (((uintptr_t)woff | (uintptr_t)toff | (uintptr_t)bad_index) & 7)
      return fail(AMPH_E_PARAM, "device offset tables and verdict arrays must be 8-byte aligned");
    if (!c->sub.empty()) c = c->sub[0];
    HIP_TRY(use_device(c->device));
    hipStream_t s = (hipStream_t)stream;
    if (!(flags & AMPH_F_ACCUMULATE)) HIP_TRY(hipMemsetAsync(bad_index, 0x7F, 8 * K, s));
    // the word table is the device's: every record takes 37 characters of the
    // texts, so T <= texts_len / 37 bounds the grid (surplus workgroups exit)
    const size_t tbound = texts_len / 37 + 1;
    hipError_t e = amph::launch_convert_share_json_seg(
        texts, woff, toff, K, amph::wire_tile_grid(tbound, K, amph::kConvTileWords), (const uint4*)tuples, alpha,
        use_zero, (uint4*)out, (unsigned long long*)bad_index, c->f, cfg(c, s, tbound));
    return e == hipSuccess ? AMPH_OK : hip_fail(e, "k_conv_json_seg");
  }
  if (int st = check_word_table(woff, K)) return st;
  std::vector<uint64_t> itoff(K);
  size_t chars = 0;
  for (size_t o = 0; o < K; ++o) {
    const uint64_t nc = amph::masked_input_data_chars(woff[o + 1] - woff[o]), end = toff[o] + nc;
    if (end < toff[o] || end > (uint64_t)texts_len)
      return fail(AMPH_E_PARAM, "object " + std::to_string(o) + ": its text [" + std::to_string(toff[o]) + ", " +
                                    std::to_string(end) + ") runs past the " + std::to_string(texts_len) +
                                    " characters of the texts");
    chars += (toff[o] - chars) & 15;  // the image keeps every text's alignment
    itoff[o] = chars;
    chars += nc;
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
  if (check_ctx(c)) return AMPH_E_PARAM;
  AMPH_NO_HOST_IO(flags);
  if (K == 0) return AMPH_OK;
  if (int st = wire_batch_parties(odos, n)) return st;
  if (!woff || !toff || !ooff || !out_text || !first_fail || !bad_char)
    return fail(AMPH_E_PARAM, "null offsets table, output text or verdict array");
  for (int j = 1; j < n; ++j)
    if (odos[j].nchars != odos[0].nchars)
      return fail(AMPH_E_LEN, "party " + std::to_string(j) + ": field buffers of " + std::to_string(odos[j].nchars) +
                                  " characters, party 0's hold " + std::to_string(odos[0].nchars));
  const size_t nchars = odos[0].nchars;
  if (flags & AMPH_F_DEVICE) {
    amph::TextSet tx{};
    for (int j = 0; j < n; ++j)
      for (int k = 0; k < 5; ++k) {
        tx.t[k][j] = b64_field(odos[j], k);
        if (nchars && !tx.t[k][j]) return fail(AMPH_E_PARAM, "null ODO field text");
        if (int st = check_dev_words({tx.t[k][j]})) return st;
      }
    if (int st = check_dev_words({secrets, out_text})) return st;
    if (((uintptr_t)woff | (uintptr_t)toff | (uintptr_t)ooff | (uintptr_t)first_fail | (uintptr_t)bad_char) & 7)
      return fail(AMPH_E_PARAM, "device offset tables and verdict arrays must be 8-byte aligned");
    if (nchars && !secrets) return fail(AMPH_E_PARAM, "null secrets");
    if (!c->sub.empty()) c = c->sub[0];
    HIP_TRY(use_device(c->device));
    hipStream_t s = (hipStream_t)stream;
    if (!(flags & AMPH_F_ACCUMULATE)) {
      HIP_TRY(hipMemsetAsync(first_fail, 0x7F, 8 * K, s));
      HIP_TRY(hipMemsetAsync(bad_char, 0x7F, 8 * K, s));
    }
    // T <= 3 nchars / 64 bounds the grid, as amph_mask_input_b64_packed; the
    // launch runs for nchars == 0 too: every object is empty and gets its "[]"
    const size_t tbound = 3 * (nchars / 64) + 3, grid = amph::wire_tile_grid(tbound, K);
    hipError_t e = amph::launch_mask_json_seg(tx, n, woff, toff, ooff, K, grid, (const uint4*)secrets, out_text,
                                              (unsigned long long*)first_fail, (unsigned long long*)bad_char,
                                              c->f, cfg(c, s, tbound));
    return e == hipSuccess ? AMPH_OK : hip_fail(e, "k_mask_json_seg");
  }
  if (int st = check_wire_tables(woff, toff, K, nchars)) return st;
  for (size_t o = 0; o < K; ++o) {
    const uint64_t end = ooff[o] + amph::masked_input_data_chars(woff[o + 1] - woff[o]);
    if (ooff[o] % 16)
      return fail(AMPH_E_PARAM, "out_text_offsets[" + std::to_string(o) + "] = " + std::to_string(ooff[o]) +
                                    " must be a multiple of 16");
    if (end < ooff[o] || end > (o + 1 < K ? ooff[o + 1] : (uint64_t)out_cap))
      return fail(AMPH_E_PARAM, "object " + std::to_string(o) + ": its output text [" + std::to_string(ooff[o]) +
                                    ", " + std::to_string(end) + ") runs past " +
                                    (o + 1 < K ? "the next slot at " + std::to_string(ooff[o + 1])
                                               : "the output capacity " + std::to_string(out_cap)));
  }
  const size_t T = woff[K];
  if (T) {
    for (int j = 0; j < n; ++j)
      for (int k = 0; k < 5; ++k)
        if (!b64_field(odos[j], k)) return fail(AMPH_E_PARAM, "null ODO field text");
    if (!secrets) return fail(AMPH_E_PARAM, "null secrets");
  }
  WirePieces io;
  io.text = [&](int j, int k, size_t o) { return b64_field(odos[j], k) + toff[o]; };
  io.secrets = [&](size_t o) { return secrets + 16 * woff[o]; };
  io.out_text = [&](size_t o) { return out_text + ooff[o]; };
  const size_t used = toff[K - 1] + amph::wire_text_chars(woff[K] - woff[K - 1]);  // the last text's end
  return wire_batch_host(c, n, K, woff, toff, used, true, false, false, io, first_fail, bad_char, true);
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
// respondtiles.hpp).  Host mode as the calls above: ONE page-locked image in
// -- [word table | text table | reject | 5 word arrays] -- and one back -- the
// five field buffers up to the last text's end -- scattered text by text, so
// the caller's gaps stay untouched; a call that fits the small-call arena is
// built and encoded there in place.  No verdicts: nothing to take back.
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
  const size_t T = woff[K];
  if (!c->sub.empty()) c = c->sub[0];
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(use_device(c->device));
  hipStream_t s;
  if (int st = host_stream(c, 0, &s)) return st;
  const size_t fchars = align256(used), fbytes = align256(16 * T);
  const size_t tab_w = 0, tab_t = tab_w + align256(8 * (K + 1)), rej = tab_t + align256(8 * K);
  const size_t wrd = rej + (reject ? align256(8 * K) : 0), in_bytes = wrd + 5 * fbytes;
  const size_t txt = in_bytes, total = txt + 5 * fchars;
  const bool small = small_call(c, total);
  uint8_t *himg, *dimg;
  if (small) {
    if (c->small.ensure(total + 256) != hipSuccess) return fail(AMPH_E_NOMEM, "small-call arena");
    himg = dimg = (uint8_t*)c->small.p;
  } else {
    if (c->wire_img.ensure(total) != hipSuccess) return fail(AMPH_E_NOMEM, "respond batch image");
    if (dev_ensure(c, c->wire, total) != hipSuccess) return fail(AMPH_E_NOMEM, "respond staging");
    himg = (uint8_t*)c->wire_img.p;
    dimg = (uint8_t*)c->wire.p;
  }
  std::memcpy(himg + tab_w, woff, 8 * (K + 1));
  std::memcpy(himg + tab_t, toff, 8 * K);
  if (reject) {  // the device's convention: kNoFail = clean
    unsigned long long* r = (unsigned long long*)(himg + rej);
    for (size_t o = 0; o < K; ++o) r[o] = reject[o] >= 0 ? (unsigned long long)reject[o] : amph::kNoFail;
  }
  const uint8_t* din[5];
  char* dout[5];
  for (int k = 0; k < 5; ++k) {
    for (size_t o = 0; o < K; ++o)
      if (const size_t w = woff[o + 1] - woff[o])
        std::memcpy(himg + wrd + k * fbytes + 16 * woff[o], io.in(k, o), 16 * w);
    din[k] = dimg + wrd + k * fbytes;
    dout[k] = (char*)(dimg + txt + k * fchars);
  }
  if (!small) {  // page-locked image, idle stream: one blocking copy (kPageableRule)
    HIP_TRY(hipMemcpy(dimg, himg, in_bytes, hipMemcpyHostToDevice));
    c->respond_copies.fetch_add(1, std::memory_order_relaxed);
  }
  hipError_t e = amph::launch_odo_b64_seg(din, dout, (const uint64_t*)(dimg + tab_w), (const uint64_t*)(dimg + tab_t),
                                          K, amph::wire_tile_grid(T, K), T, used,
                                          reject ? (const unsigned long long*)(dimg + rej) : nullptr, cfg(c, s, T));
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(s);
    return hip_fail(e, "k_odo_b64_seg");
  }
  HIP_TRY(hipStreamSynchronize(s));
  if (!small) {
    HIP_TRY(hipMemcpy(himg + txt, dimg + txt, total - txt, hipMemcpyDeviceToHost));
    c->respond_copies.fetch_add(1, std::memory_order_relaxed);
  }
  for (int k = 0; k < 5; ++k)
    for (size_t o = 0; o < K; ++o)
      if (const size_t nc = amph::wire_text_chars(woff[o + 1] - woff[o]))
        std::memcpy(io.out(k, o), himg + txt + k * fchars + toff[o], nc);
  return AMPH_OK;
}
}  // namespace

extern "C" {

uint64_t amph_respond_batch_copies(const amph_ctx* c) {
  if (!c) return 0;
  return (c->sub.empty() ? c : c->sub[0])->respond_copies.load(std::memory_order_relaxed);
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
    if (((uintptr_t)woff | (uintptr_t)toff | (uintptr_t)reject) & 7)
      return fail(AMPH_E_PARAM, "device offset tables and verdict arrays must be 8-byte aligned");
    if (!c->sub.empty()) c = c->sub[0];
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
