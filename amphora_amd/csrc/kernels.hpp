// Launch interface of the share-arithmetic kernels (internal to libamphora_hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "field.hpp"

namespace amph {

constexpr int kMaxParties = 16;
constexpr int kMaxBlock = 1024;  // kernels accept any block size <= this
// first_fail sentinel: what hipMemsetAsync(.., 0x7F, 8) leaves behind.
constexpr unsigned long long kNoFail = 0x7F7F7F7F7F7F7F7FULL;

// SoA word arrays of one OutputDeliveryObject set: f[field][party], field
// order y (secretShares), r, v, w, u.  Each points at 16-byte words.
struct OdoSet {
  const uint4* f[5][kMaxParties];
};

struct ShareSet {
  const uint4* s[kMaxParties];
};

// The exchange decode's SPAN FORM (launch_exchange_decode_spans): the values
// of 8 KiB span s of the text, in text order, at slots [kXSpanSlots s, ...);
// neg byte per slot = sign (bit 0) | key "b" (bit 1).  base[s] = the index of
// span s's first value (bits 0..39), base[nb] = the total; when base[nb]
// carries bits above 39 or its count is not the pair count x 2, the general
// pass wrote the values in pair order instead (slot = value index).  map[b]
// = the window of values [kXMapValues b, kXMapValues (b + 1)) (one
// k_open_post workgroup's): x = s0, the span holding its first value, y = that
// value's rank in s0, z = o1 | o2 << 16, w = o3 with o_i = base[s0 + i] -
// kXMapValues b (0xFFFF / ~0 past the last span): value kXMapValues b + t
// lies in span s0 + i for o_i <= t < o_(i+1) (o_0 = -y).
constexpr size_t kXSpanBytes = 8192;
constexpr int kXSpanSlots = 528;  // 33 x 256 B per span: not a power-of-two stride (see k_xdec_span)
constexpr size_t kXMapValues = 256;
struct XSpans {
  uint4* mag;
  uint8_t* neg;
  uint64_t* base;  // nb + 1 words
  uint4* map;      // xspan_map_words(npairs) windows
  size_t nb;       // xspan_spans(len)
};

struct SignedSet {  // per party: diff magnitudes (2 words per pair) + sign words
  const uint4* mag[kMaxParties];
  const uint32_t* neg[kMaxParties];  // 4 sign bytes per source word (see K_ODO_PRE)
  // span form (k_open_post only): base / map / nb of the party's XSpans, null
  // for pair-ordered diffs (amph_odo_pre's layout)
  const uint64_t* sbase[kMaxParties];
  const uint4* smap[kMaxParties];
  size_t snb[kMaxParties];
};

struct TextSet {  // base64 text of each ODO field: t[field][party], 16-byte aligned
  const char* t[5][kMaxParties];
};

struct LaunchCfg {
  hipStream_t stream;
  int grid_cap;  // 0 = full grid (one word per thread); > 0 caps it (grid-stride beyond)
  int block;     // threads per workgroup, multiple of 64, <= kMaxBlock
  hipEvent_t ev_start = nullptr;  // optional: stamped by the kernel dispatch itself
  hipEvent_t ev_stop = nullptr;
  size_t base = 0;  // host pipeline: the batch's first word within the call (0 elsewhere)
};

// K_RV: recombine 5 fields over n parties, verify w == y r, u == v r,
// write canonical y (LE16) and atomic-min the first failing index.
hipError_t launch_recombine_verify(const OdoSet& odo, int n, size_t words, uint4* out_y,
                                   unsigned long long* first_fail, const Fp& f, const LaunchCfg& c);

// K_MASK: K_RV over Input Mask ODOs fused with maskInput:
// out[i] = [s_i] - [m_i] for i < n_secrets (s_i any 128-bit LE integer).
hipError_t launch_mask_input(const OdoSet& odo, int n, size_t words, const uint4* secrets,
                             size_t n_secrets, uint4* out_masked, unsigned long long* first_fail,
                             const Fp& f, const LaunchCfg& c);

// Segmented K_RV / K_MASK over a packed layout: every field of every party is
// the concatenation of n_objects objects' words, object o owning words
// [offsets[o], offsets[o + 1]) (seglookup.hpp; device table of n_objects + 1
// words).  first_fail is an array of n_objects words: a failing global word g
// of object o min-combines g - offsets[o] into first_fail[o].  The launch
// covers global words [ibase, ibase + words) -- the array pointers are those
// of word ibase.  One secret per word for the mask form (no verify-only tail).
hipError_t launch_recombine_verify_seg(const OdoSet& odo, int n, size_t words, uint4* out_y,
                                       unsigned long long* first_fail, const uint64_t* offsets,
                                       size_t n_objects, size_t ibase, const Fp& f, const LaunchCfg& c);
hipError_t launch_mask_input_seg(const OdoSet& odo, int n, size_t words, const uint4* secrets,
                                 uint4* out_masked, unsigned long long* first_fail,
                                 const uint64_t* offsets, size_t n_objects, size_t ibase, const Fp& f,
                                 const LaunchCfg& c);

// recombineObject for one field: canonical sum_j fromGfp(share_j).
hipError_t launch_recombine(const ShareSet& sh, int n, size_t words, uint4* out, const Fp& f,
                            const LaunchCfg& c);

// verifySecrets on canonical (LE16) integers: y r == w and v r == u (mod p).
// min-combine a one-word call's verdict (index 0 or kNoFail) as word `base`
hipError_t launch_ff_merge(unsigned long long* ff, const unsigned long long* tail, size_t base,
                           hipStream_t s);

hipError_t launch_verify(const uint4* y, const uint4* r, const uint4* u, const uint4* v,
                         const uint4* w, size_t words, unsigned long long* first_fail,
                         const Fp& f, const LaunchCfg& c);

// K_CONV: masked (16 B) + input-mask tuple (value||mac, 32 B) -> share (value||mac).
hipError_t launch_convert_share(const uint4* masked, const uint4* tuples, size_t words,
                                W4 alpha_mont, int use_zero_input, uint4* out, const Fp& f,
                                const LaunchCfg& c);

// K_CONV from the MaskedInput "data" array text (37 words + 1 characters, any
// byte alignment; "[]" for no words): bad = min byte offset of an offending
// frame byte or base64 character; the output is unspecified when it is set.
hipError_t launch_convert_share_json(const char* text, const uint4* tuples, size_t words, W4 alpha_mont,
                                     int use_zero_input, uint4* out, unsigned long long* bad,
                                     const Fp& f, const LaunchCfg& c);

// K_ODO_PRE: raw y/r/v copies (each optional) + signed Beaver diffs; with
// lens, also the exchange text length of every kXLenPairs FactorPairs
// (launch_exchange_encode_lens' input).
constexpr size_t kXLenPairs = 128;
hipError_t launch_odo_pre(const uint4* share_data, int share_stride_words, const uint4* masks,
                          const uint4* triples, size_t words, uint4* out_y, uint4* out_r,
                          uint4* out_v, uint4* out_mag, uint32_t* out_neg, const Fp& f,
                          const LaunchCfg& c, uint64_t* lens = nullptr);

// recombineDiffs: sum over parties of signed diffs mod p -> canonical opened values.
hipError_t launch_open_diffs(const SignedSet& d, int n, size_t pairs, uint4* out_opened,
                             const Fp& f, const LaunchCfg& c);

// K_ODO_POST: Beaver product shares from opened (D, E) + triples -> w, u wire words.
hipError_t launch_odo_post(const uint4* opened, const uint4* triples, size_t words,
                           int is_player0, uint4* out_w, uint4* out_u, const Fp& f,
                           const LaunchCfg& c);

// recombineDiffs + K_ODO_POST in one launch: every party's signed diffs
// (SignedSet) + triples -> w, u wire words; the opened D, E stay in registers.
hipError_t launch_open_post(const SignedSet& d, int n, const uint4* triples, size_t words,
                            int is_player0, uint4* out_w, uint4* out_u, const Fp& f,
                            const LaunchCfg& c, bool stage_mag = false);

// toGfp / fromGfp over word arrays; maskInput with canonical masks.
hipError_t launch_to_gfp(const uint4* in, size_t words, uint4* out, const Fp& f, const LaunchCfg& c);
hipError_t launch_from_gfp(const uint4* in, size_t words, uint4* out, const Fp& f, const LaunchCfg& c);
hipError_t launch_mask_words(const uint4* secrets, const uint4* masks, size_t words, uint4* out,
                             const Fp& f, const LaunchCfg& c);

// base64 wire codec (codec.hip): standard alphabet, '=' padding, no line breaks.
hipError_t launch_b64_encode(const uint8_t* in, size_t nbytes, char* out, const LaunchCfg& c);
// n <= 5 streams of nbytes each, one launch
hipError_t launch_b64_encode_multi(const uint8_t* const* in, char* const* out, int n, size_t nbytes,
                                   const LaunchCfg& c);
// Many objects' five ODO fields in one launch (include/amphora_respond_batch.h;
// respondtiles.hpp): in[k] = field k's packed words (total_words of them, the
// objects on woff[n_objects + 1]), out[k] = its slotted text buffer of nchars
// characters (object o's text at toff[o]); all ten 16-byte aligned.  reject:
// null, or n_objects words -- an object whose word is not kNoFail gets "!!!!"
// as its texts' first four characters.  grid: wire_tile_grid(T, n_objects)
// workgroups, or any upper bound of it (surplus workgroups exit).
hipError_t launch_odo_b64_seg(const uint8_t* const* in, char* const* out, const uint64_t* woff,
                              const uint64_t* toff, size_t n_objects, size_t grid, uint64_t total_words,
                              uint64_t nchars, const unsigned long long* reject, const LaunchCfg& c);
// text_end: the range ends the text, so '=' may pad its last two chars;
// out_bytes = kB64PadOnDevice (with text_end): the kernel sizes the output
// from the text's last two characters itself, no host read-back
constexpr size_t kB64PadOnDevice = ~(size_t)0;
hipError_t launch_b64_decode(const char* in, size_t nchars, uint8_t* out, size_t out_bytes,
                             unsigned long long* bad, const LaunchCfg& c, bool text_end = true);
hipError_t launch_b64_words(const uint4* in, size_t words, char* out, const LaunchCfg& c);
hipError_t launch_b64_unwords(const char* in, size_t words, uint4* out, unsigned long long* bad,
                              const LaunchCfg& c);

// Beaver open exchange codec (exchange.hip): FactorPair JSON array <-> signed
// diffs (mag 16 B + sign byte per value, 2 values per pair).
size_t xenc_scratch_bytes(size_t npairs);
size_t xenc_max_bytes(size_t npairs);
hipError_t launch_exchange_encode(const uint4* mag, const uint8_t* neg, size_t npairs, char* out,
                                  unsigned long long* out_len, void* scratch, const LaunchCfg& c);
// the same text when K_ODO_PRE has written the lengths of every kXLenPairs
// pairs (lens: ceil(npairs / kXLenPairs) + 1 words, scanned in place)
size_t xenc_lens_scratch_bytes(size_t npairs);
hipError_t launch_exchange_encode_lens(const uint4* mag, const uint8_t* neg, size_t npairs, uint64_t* lens,
                                       char* out, unsigned long long* out_len, void* scratch, const LaunchCfg& c);
size_t xdec_scratch_bytes(size_t len);
hipError_t launch_exchange_decode(const char* text, size_t len, size_t npairs, uint4* mag,
                                  uint8_t* neg, unsigned long long* bad, void* scratch,
                                  const LaunchCfg& c);
// decode into span form (see XSpans): one read of the text, no count pass;
// resets *bad itself (kNoFail) before reporting into it
size_t xspan_spans(size_t len);
size_t xspan_slots(size_t len, size_t npairs);  // >= both the span slots and 2 npairs
size_t xspan_map_words(size_t npairs);
size_t xdec_spans_scratch_bytes(size_t len);
hipError_t launch_exchange_decode_spans(const char* text, size_t len, size_t npairs, const XSpans& out,
                                        unsigned long long* bad, void* scratch, const LaunchCfg& c);

// Many objects' exchange texts per call (include/amphora_exchange_batch.h;
// exchangetiles.hpp): the diffs of object o are pairs [pair_offsets[o],
// pair_offsets[o + 1]) of the packed arrays, its text lies at text_offsets[o]
// (a multiple of 8192) of ONE 16-byte-aligned buffer.  Device tables; a fixed
// number of launches whatever n_objects >= 1 is.
//   encode: out_lens[o] = the text's length; nothing of out[0, out_cap) outside
// the texts is written.
//   decode: bad[o] min-combines object o's first offending offset inside its
// own text (text_lens[o] on a count mismatch); reset_bad: set to kNoFail first.
size_t xencs_scratch_bytes(size_t npairs, size_t n_objects);
hipError_t launch_exchange_encode_seg(const uint4* mag, const uint8_t* neg, size_t npairs,
                                      const uint64_t* pair_offsets, const uint64_t* text_offsets,
                                      size_t n_objects, char* out, size_t out_cap, unsigned long long* out_lens,
                                      void* scratch, const LaunchCfg& c);
size_t xdecs_scratch_bytes(size_t texts_len, size_t n_objects);
hipError_t launch_exchange_decode_seg(const char* texts, size_t texts_len, const uint64_t* pair_offsets,
                                      const uint64_t* text_offsets, const uint64_t* text_lens, size_t n_objects,
                                      size_t npairs, uint4* mag, uint8_t* neg, unsigned long long* bad,
                                      bool reset_bad, void* scratch, const LaunchCfg& c);

// Many objects' partner texts in SPAN FORM (include/amphora_party_batch.h;
// partytiles.hpp): the texts lie at text_offsets[o] of one 16-byte-aligned
// buffer as above.  mag / neg: kXSpanSlots slots per 8 KiB span of the BUFFER
// (nb = texts_len / 8192 + 1 spans), the values of buffer span s in text order
// from slot kXSpanSlots s; base[nb + 1]: the scanned count words.  Object o is
// in span form iff base[span0 + spans] - base[span0] == 2 P_o; any other
// object's values are written in pair order into rows [2 pair_offsets[o], ...)
// of pmag / pneg (2 npairs rows; byte = sign), for that object alone.
// win[party_tile_grid(npairs, n_objects)]: the window of every open-post
// tile, x = kPartyPairOrder for a tile of an object in pair order.
// bad[o]: reset, then object o's verdict as launch_exchange_decode_seg's.
struct XSpansSeg {
  uint4* mag;
  uint8_t* neg;
  uint64_t* base;
  uint4* pmag;
  uint8_t* pneg;
  uint4* win;
  size_t nb;
};
size_t xspans_seg_scratch_bytes(size_t texts_len);
hipError_t launch_exchange_decode_spans_seg(const char* texts, size_t texts_len, const uint64_t* pair_offsets,
                                            const uint64_t* text_offsets, const uint64_t* text_lens,
                                            size_t n_objects, size_t npairs, const XSpansSeg& out,
                                            unsigned long long* bad, void* scratch, const LaunchCfg& c);

// launch_open_post over many objects (partytiles.hpp): one workgroup per
// 128-pair tile that never straddles two objects.  Party 0's diffs are pair
// ordered (K_ODO_PRE's arrays over the concatenation); parties 1 .. n-1 are
// partners decoded by launch_exchange_decode_spans_seg (span[j], verdict[j] =
// the n_objects verdict words of that decode).  w and u are stored at the
// packed word positions; the tile of an object's first pairs also writes
// reject[object] = the smallest of the partners' verdict words for it
// (kNoFail without partners; an object of no pairs keeps no tile and its word
// is not written).  Tables are device arrays.
struct PartySegSet {
  const uint4* mag0;
  const uint32_t* neg0;
  XSpansSeg span[kMaxParties];
  const unsigned long long* verdict[kMaxParties];
  const uint64_t *pair_offsets, *text_offsets;
  size_t n_objects;
  uint64_t npairs;
  unsigned long long* reject;
};
hipError_t launch_open_post_seg(const PartySegSet& d, int n, const uint4* triples, int is_player0, uint4* out_w,
                                uint4* out_u, const Fp& f, const LaunchCfg& c);

// Synthetic honest n-party ODOs (bench/test input generator, device-side).
struct OutSet {
  uint4* f[5][kMaxParties];
};
hipError_t launch_synth_odos(const OutSet& out, int n, size_t words, uint64_t seed,
                             uint4* out_plain_y, long long fault_index, int noncanon_permille,
                             const Fp& f, const LaunchCfg& c);
hipError_t launch_synth_words(uint4* out, size_t count, uint64_t seed, const Fp& f,
                              const LaunchCfg& c);
// K_RV / K_MASK straight from the wire: the parties' base64 ODO fields
// (nchars each = 4 ceil(16 words / 3), `pad` '=' at the end) decoded in the
// workgroup; bad = min (5 party + field) * nchars + offset of an invalid char.
hipError_t launch_rv_b64(const TextSet& tx, int n, size_t words, size_t nchars, uint32_t pad,
                         uint4* out_y, unsigned long long* first_fail, unsigned long long* bad,
                         const Fp& f, const LaunchCfg& c);
hipError_t launch_mask_b64(const TextSet& tx, int n, size_t words, size_t nchars, uint32_t pad,
                           const uint4* secrets, size_t n_secrets, uint4* out16, char* out24,
                           unsigned long long* first_fail, unsigned long long* bad, const Fp& f,
                           const LaunchCfg& c);
// launch_mask_b64 with the records framed as the MaskedInput "data" array
// text: out_text (16-byte aligned) gets 37 n_secrets + 1 characters; n_secrets
// in [1, words] (the caller writes "[]" for none)
hipError_t launch_mask_json(const TextSet& tx, int n, size_t words, size_t nchars, uint32_t pad,
                            const uint4* secrets, size_t n_secrets, char* out_text,
                            unsigned long long* first_fail, unsigned long long* bad, const Fp& f,
                            const LaunchCfg& c);

// The client session (include/amphora_client_session.h; wire.hip, "one party
// at a time"): five running sums of canonical Montgomery words, `words` each.
struct SumSet {
  uint4* s[5];  // y, r, v, w, u
};
// ONE party's five texts (tx.t[k][0]) decoded in the workgroup and added into
// the sums (not atomic: launches of one session run in order on one stream);
// bad_session / bad_call (the latter may be null) min-combine the whole
// call's (5 party + field) * nchars + offset of an invalid character.
hipError_t launch_acc_b64(const TextSet& tx, int party, size_t words, size_t nchars, uint32_t pad,
                          const SumSet& sums, unsigned long long* bad_session, unsigned long long* bad_call,
                          const Fp& f, const LaunchCfg& c);
// launch_mask_b64 (out_text null) / launch_mask_json (out_text set, n_secrets
// >= 1) with the summed fields read from the session's sums; every one of the
// `words` masks is verified, n_secrets <= words.
hipError_t launch_mask_sums(const SumSet& sums, size_t words, const uint4* secrets, size_t n_secrets, uint4* out16,
                            char* out24, char* out_text, unsigned long long* first_fail, const Fp& f,
                            const LaunchCfg& c);
// The same two for K objects (include/amphora_client_batch.h): ONE party's
// five slotted field buffers (the layout of launch_rv_b64_seg: object o's
// texts at toff[o], its words packed on woff[n_objects + 1]) added into sums
// packed on woff; bad_session / bad_call (the latter may be null) are arrays
// of n_objects words, [o] min-combines (5 party + field) * nchars_o + offset.
// launch_mask_sums_seg: secrets, out16 / out24 packed on woff, one secret per
// mask word, or (out_text set) object o's framed text at out_text + ooff[o];
// first_fail an array of n_objects words with object-local indices.  grid:
// wire_tile_grid(T, n_objects) or any upper bound of it.  Device tables.
hipError_t launch_acc_b64_seg(const TextSet& tx, int party, const uint64_t* woff, const uint64_t* toff,
                              size_t n_objects, size_t grid, const SumSet& sums, unsigned long long* bad_session,
                              unsigned long long* bad_call, const Fp& f, const LaunchCfg& c);
hipError_t launch_mask_sums_seg(const SumSet& sums, const uint64_t* woff, const uint64_t* ooff, size_t n_objects,
                                size_t grid, const uint4* secrets, uint4* out16, char* out24, char* out_text,
                                unsigned long long* first_fail, const Fp& f, const LaunchCfg& c);
// launch_acc_b64_seg on the texts where a party's response bodies hold them
// (include/amphora_client_bodies.h; bodyspans.hpp): `buffer` is 16-byte
// aligned device memory whose allocation reaches the next multiple of 16 past
// the last text, starts[5][n_objects] (a device table) gives the byte where
// object o's field k begins -- any residue mod 16 -- or ~0 in field 0 for an
// object that is absent: it reports (5 party) * nchars_o and adds nothing.
// Only aligned 16-byte granules that hold text are read.
hipError_t launch_acc_b64_bodies(const char* buffer, int party, const uint64_t* woff, const uint64_t* starts,
                                 size_t n_objects, size_t grid, const SumSet& sums, unsigned long long* bad_session,
                                 unsigned long long* bad_call, const Fp& f, const LaunchCfg& c);

// K_RV / K_MASK from the wire for many objects in one launch (wire.hip, "the
// slotted text layout"; wiretiles.hpp): object o's texts start toff[o]
// characters into every field buffer and its words are packed on
// woff[n_objects + 1]; ff / bad are arrays of n_objects verdict words with
// object-local indices.  grid: wire_tile_grid(T, n_objects) workgroups, or
// any upper bound of it (surplus workgroups exit).  One secret per mask word.
hipError_t launch_rv_b64_seg(const TextSet& tx, int n, const uint64_t* woff, const uint64_t* toff,
                             size_t n_objects, size_t grid, uint4* out_y, unsigned long long* first_fail,
                             unsigned long long* bad, const Fp& f, const LaunchCfg& c);
hipError_t launch_mask_b64_seg(const TextSet& tx, int n, const uint64_t* woff, const uint64_t* toff,
                               size_t n_objects, size_t grid, const uint4* secrets, uint4* out16, char* out24,
                               unsigned long long* first_fail, unsigned long long* bad, const Fp& f,
                               const LaunchCfg& c);

// Many MaskedInput uploads per launch (include/amphora_upload_batch.h).
// Party side: K "data" array texts, object o's at text + toff[o] (any byte
// alignment), its tuples and shares rows [woff[o], woff[o + 1]) of the packed
// arrays; bad[o] = the smallest offending byte offset inside object o's own
// text.  grid: wire_tile_grid(T, n_objects, 128) or any upper bound of it.
hipError_t launch_convert_share_json_seg(const char* text, const uint64_t* woff, const uint64_t* toff,
                                         size_t n_objects, size_t grid, const uint4* tuples, W4 alpha_mont,
                                         int use_zero_input, uint4* out, unsigned long long* bad, const Fp& f,
                                         const LaunchCfg& c);
// Client side: launch_mask_b64_seg with object o's records written as its
// framed "data" array text at out_text + ooff[o] (ooff[o] a multiple of 16;
// "[]" for an object of no words).  grid: wire_tile_grid(T, n_objects).
hipError_t launch_mask_json_seg(const TextSet& tx, int n, const uint64_t* woff, const uint64_t* toff,
                                const uint64_t* ooff, size_t n_objects, size_t grid, const uint4* secrets,
                                char* out_text, unsigned long long* first_fail, unsigned long long* bad,
                                const Fp& f, const LaunchCfg& c);

// Small host calls: copy n verdict words from device memory to page-locked
// host memory and reset them to kNoFail (one 64-lane workgroup).
hipError_t launch_take_words(unsigned long long* dev, unsigned long long* host, int n, hipStream_t s);
// Packed small host calls: n verdict words (any n) to page-locked host memory.
hipError_t launch_take_array(const unsigned long long* dev, unsigned long long* host, size_t n, hipStream_t s);

// Device-mode party session: poison the five base64 fields ("!!!!" as their
// first unit) when any partner verdict word is not kNoFail (one workgroup).
struct PoisonB64 {
  const unsigned long long* bad[16];
  int n_bad;
  char* field[5];
  size_t chars;  // characters per field
};
hipError_t launch_poison_b64(const PoisonB64& a, hipStream_t s);

// Measurement only: K_MASK's memory pattern without the arithmetic.
hipError_t launch_stream_probe(const OdoSet& odo, int n, size_t words, const uint4* secrets,
                               uint4* out, const LaunchCfg& c);

}  // namespace amph
