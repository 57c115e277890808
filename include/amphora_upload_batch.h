/*
 * amphora_upload_batch.h -- extension of amphora.h and amphora_wire_batch.h:
 * the Input Supply upload for MANY MaskedInput bodies in one launch, both
 * ends, on the framed "data" array text itself.
 *
 * Party side: amph_convert_share_json takes one POST body's "data" text per
 * launch; a party is where many clients' POST /masked-inputs requests
 * converge (MaskedInputController.upload -> StorageService.createSecret ->
 * service SecretShareUtil.convertToSecretShare, SecretShareUtil.java:58-107).
 * amph_convert_share_json_packed / _batch check, decode and convert K such
 * texts in one launch, one verdict per text.
 * Client side: amph_mask_input_b64_packed / _batch return packed 24-character
 * records that the host still has to frame K times; amph_mask_input_json_packed
 * / _batch write each secret's framed text ([{"value":"..."},...],
 * MaskedInput.java:25-62, MaskedInputData.java:44-52) in the kernel, as
 * amph_mask_input_json does for one.
 * Same conventions as amphora.h (status codes, flags, amph_last_error,
 * threading).  A words-only amph_convert_share needs no packed form: it has
 * no verdict, so one call on the concatenation of the objects' words and
 * tuples already is the packed form.
 */
#ifndef AMPHORA_UPLOAD_BATCH_H_
#define AMPHORA_UPLOAD_BATCH_H_

#include "amphora.h"
#include "amphora_wire_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- common to the PACKED calls ----------------------------------------------
 *   word_offsets[n_objects + 1]: the packed calls' table (offsets[0] = 0,
 *   nondecreasing, last entry T).  Object o has W_o = word_offsets[o + 1] -
 *   word_offsets[o] words and a "data" array text of
 *   amph_masked_input_data_chars(W_o) characters: '[' + one 37-byte record per
 *   word (its trailing ',' / ']' included), or "[]" for no words.
 *   amph_upload_slot_chars(words) = that length rounded up to 16, the stride
 *   of the dense 16-byte-aligned layout the mask side writes.
 *
 *   Per object, bad_index[o] / first_fail[o] / bad_char[o], the share rows and
 *   the text are bit-identical to the single call (amph_convert_share_json /
 *   amph_mask_input_json) on that object alone.  An object with a reported
 *   text fault (bad_index[o] >= 0, bad_char[o] >= 0) has unspecified output
 *   inside its own rows / its own text only; every other object's output is
 *   written.
 *
 *   Host mode moves ONE page-locked image to the device (tables, texts or
 *   field buffers, tuples or secrets) and one back (shares or texts, and the
 *   verdicts), whatever n_objects is; a call that fits the small-call arena
 *   is built there and moves nothing (amph_upload_batch_copies counts).
 *
 *   AMPH_F_DEVICE: the tables and the verdict arrays are device arrays, 8-byte
 *   aligned; tuples, shares, secrets, field buffers and out_text 16-byte
 *   aligned (the convert side's `texts` at any alignment); asynchronous on
 *   `stream`.  The verdict arrays are reset to AMPH_NO_FAILURE unless
 *   AMPH_F_ACCUMULATE is set (then min-combined).  The tables' contract is the
 *   CALLER's: whatever they hold, no share row past word_offsets[n_objects]
 *   (T: the packed arrays hold that many rows) is written and nothing outside
 *   [0, n_objects) of the verdict arrays.  The convert launch is sized from
 *   texts_len (T <= texts_len / 37: the texts' lengths must not add up to
 *   more than texts_len), the mask launch from the field buffers' nchars.
 *
 *   AMPH_F_HOST_IO is refused (AMPH_E_PARAM).  A multi-device context runs
 *   these calls on devices[0].  n_objects == 0 returns AMPH_OK and launches
 *   nothing. */
size_t amph_upload_slot_chars(size_t words);

/* ---- party: K "data" array texts -> K shares ------------------------------------
 *   texts / texts_len: one buffer; object o's text starts text_offsets[o]
 *   bytes into it, at ANY alignment -- the dense concatenation is legal.  The
 *   texts need not be ordered or disjoint (they are only read).  Bytes of the
 *   buffer outside the texts may be read only within the 16-byte granules
 *   that hold text (amph_convert_share_json's rule).  Host mode checks the
 *   word table and that every text lies inside [0, texts_len): a breach
 *   returns AMPH_E_PARAM with nothing launched.
 *   mask_tuples / out_share: 32 T bytes, packed on word_offsets.  One MAC key
 *   and one use_zero_input_as_data per call (a party has one of each).
 *   bad_index[n_objects]: -1 (AMPH_NO_FAILURE in device mode) or the smallest
 *   byte offset, counted inside object o's own text, of a byte the frame or
 *   the base64 rule refuses.  Host status: AMPH_E_PARAM if any text was
 *   refused; amph_last_error names the first such object, its offset and
 *   record, and how many were refused. */
int amph_convert_share_json_packed(amph_ctx* ctx, const char* texts, size_t texts_len,
                                   const uint64_t* word_offsets, const uint64_t* text_offsets,
                                   size_t n_objects, const uint8_t* mask_tuples, const uint8_t mac_key_le[16],
                                   int use_zero_input_as_data, uint8_t* out_share, int64_t* bad_index,
                                   uint32_t flags, void* stream);

/* GATHER form, host memory only (any flag: AMPH_E_PARAM): texts[o] of lens[o]
 * characters, mask_tuples[o] / out_share[o] of 32 words[o] bytes.  lens[o] !=
 * amph_masked_input_data_chars(words[o]) gives AMPH_E_LEN naming the object,
 * before any GPU work.  The library concatenates the texts and tuples in
 * page-locked memory, runs the packed path once and scatters the shares. */
int amph_convert_share_json_batch(amph_ctx* ctx, const char* const* texts, const size_t* lens,
                                  const size_t* words, size_t n_objects, const uint8_t* const* mask_tuples,
                                  const uint8_t mac_key_le[16], int use_zero_input_as_data,
                                  uint8_t* const* out_share, int64_t* bad_index, uint32_t flags);

/* ---- client: K secrets -> K framed "data" array texts ---------------------------
 *   mask_odos / word_offsets / text_offsets / secrets / first_fail / bad_char:
 *   amph_mask_input_b64_packed's (amphora_wire_batch.h): the slotted base64
 *   field buffers, one secret per mask word, no verify-only tail.
 *   out_text / out_cap / out_text_offsets[n_objects]: object o's text is
 *   written at out_text + out_text_offsets[o]; every entry a multiple of 16,
 *   the slots ordered, disjoint and inside out_cap (host mode checks this:
 *   AMPH_E_PARAM, nothing launched).  Bytes of out_text outside the texts --
 *   the gaps between slots, anything after an object's ']' -- are never
 *   written.  Verdicts and host status: amph_mask_input_b64_packed's order
 *   (AMPH_E_PARAM for a bad character, else AMPH_E_VERIFY, else AMPH_OK). */
int amph_mask_input_json_packed(amph_ctx* ctx, const amph_odo_b64* mask_odos, int n_parties,
                                const uint64_t* word_offsets, const uint64_t* text_offsets,
                                size_t n_objects, const uint8_t* secrets, char* out_text, size_t out_cap,
                                const uint64_t* out_text_offsets, int64_t* first_fail, int64_t* bad_char,
                                uint32_t flags, void* stream);

/* GATHER form, host memory only (any flag: AMPH_E_PARAM): mask_odos[o *
 * n_parties + j] as amph_mask_input_b64_batch; a field nchars that does not
 * match words[o] gives AMPH_E_LEN naming object and party before any GPU work.
 * out_texts[o] receives amph_masked_input_data_chars(words[o]) characters. */
int amph_mask_input_json_batch(amph_ctx* ctx, const amph_odo_b64* mask_odos, int n_parties, size_t n_objects,
                               const size_t* words, const uint8_t* const* secrets, char* const* out_texts,
                               int64_t* first_fail, int64_t* bad_char, uint32_t flags);

/* Host-device copies (hipMemcpy calls) the host mode of the four calls above
 * has issued on this context so far: a constant number per call, whatever
 * n_objects is (0 for a call that fits the small-call arena). */
uint64_t amph_upload_batch_copies(const amph_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* AMPHORA_UPLOAD_BATCH_H_ */
