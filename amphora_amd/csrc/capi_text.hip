// C ABI of libamphora_hip (declared in include/amphora.h): the text forms --
// base64, the Beaver open exchange codec, K_RV / K_MASK from one object's wire
// texts and K_CONV from one MaskedInput "data" array text.  The many-objects
// forms of the last three are capi_batch.hip.
#include "capi_internal.hpp"

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

// Device-pointer calls of the exchange codec (the single calls here, the
// many-objects calls of capi_batch.hip) take their scan scratch from one
// per-context buffer: under the context mutex each call makes its stream wait
// for the previous call's kernels (xdev_done) before reusing it, then records
// its own.  (The device's stream-ordered pool handed two contexts overlapping
// buffers in the host paths)
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

int check_parties(const amph_odo_b64* odos, int n) {
  if (!odos || n < 1 || n > AMPH_MAX_PARTIES)
    return fail(AMPH_E_PARAM, "n_parties must be in [1, 16] with a non-null ODO array");
  return AMPH_OK;
}

int wire_bad_message(int64_t bad, size_t nchars) {
  const size_t o = (size_t)bad / nchars, at = (size_t)bad % nchars;
  return fail(AMPH_E_PARAM, "Illegal base64 character at index " + std::to_string(at) + " of party " +
                                std::to_string(o / 5) + "'s " + kOdoFieldNames[o % 5]);
}
}  // namespace capi

extern "C" {

// ---- Beaver open exchange codec ------------------------------------------------
// Host-pointer calls of the exchange codec: one shot on the context's first
// stream (the whole text is scanned at once, so there is no batching).
// Device-pointer calls take their scan scratch with dev_scratch (above).

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
// Shared checks; *nchars / *pad for `words` 16-byte words.
int wire_check(const amph_odo_b64* odos, int n, size_t words, size_t* nchars, uint32_t* pad) {
  if (int st = check_parties(odos, n)) return st;
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
