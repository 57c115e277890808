/*
 * amphora_respond_batch.h -- extension of amphora.h and amphora_wire_batch.h:
 * the base64 fields of MANY Output Delivery responses written in one launch.
 *
 * A party answers GET /secret-shares/{id} (VerifiableSecretShare) and GET
 * /input-masks (OutputDeliveryObject) with five base64 strings: secretShares,
 * rShares, vShares, wShares, uShares.  It is where many clients' requests
 * converge.  amph_odo_pre and amph_open_post have no verdict and work word by
 * word (pair 2i / 2i + 1 uses tuples and triples 2i / 2i + 1), so one call on
 * the concatenation of K requests' words already is their packed form, as
 * amphora_upload_batch.h notes for amph_convert_share.  Base64 is not: every
 * object's text has its own length, its own '=' padding and its own place.
 * amph_odo_fields_b64_packed / _batch write K objects' five texts in one
 * launch, into exactly the slotted field buffers amphora_wire_batch.h reads:
 * a party's five output buffers and the two tables go into
 * amph_recombine_verify_b64_packed / amph_mask_input_b64_packed unchanged.
 * Same conventions as amphora.h (status codes, flags, amph_last_error,
 * threading).
 */
#ifndef AMPHORA_RESPOND_BATCH_H_
#define AMPHORA_RESPOND_BATCH_H_

#include "amphora.h"
#include "amphora_wire_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* amph_odo_b64 with writable texts: one buffer per field, each of `nchars`
 * characters of capacity, holding every object's text of that field. */
typedef struct amph_odo_b64_out {
  char* secret_shares;
  char* r_shares;
  char* v_shares;
  char* w_shares;
  char* u_shares;
  size_t nchars; /* capacity of each of the five buffers */
} amph_odo_b64_out;

/* ---- PACKED form ----------------------------------------------------------------
 *   fields: ONE amph_odo whose five arrays each hold T = nbytes / 16 words, the
 *   concatenation of the objects' words (nbytes not a multiple of 16:
 *   AMPH_E_LEN).
 *   word_offsets[n_objects + 1] / text_offsets[n_objects]: the tables of
 *   amph_recombine_verify_b64_packed, word for word.  Object o has W_o =
 *   word_offsets[o + 1] - word_offsets[o] words (word_offsets[0] = 0,
 *   nondecreasing, last entry T) and a text of 4 * ceil(16 * W_o / 3)
 *   characters at text_offsets[o] of every one of the five buffers; every
 *   entry a multiple of 16, the slots ordered and disjoint, the last text ends
 *   at or before out->nchars.  amph_wire_slot_chars is the dense stride.
 *   Per object and field the text is bit-identical to amph_base64_encode of
 *   that object's 16 * W_o bytes (Jackson's MIME_NO_LINEFEEDS).  An object of 0
 *   words has an empty text: nothing is written for it.  Bytes of the buffers
 *   outside the texts -- the gaps between slots, everything after the last
 *   text -- are NEVER WRITTEN.
 *   reject: NULL, or one verdict word per object.  A rejected object gets
 *   "!!!!" as the first four characters of each of its five texts (no base64
 *   decoder accepts them: amph_recombine_verify_b64_packed reports bad_char 0
 *   for it), written by the same launch; the rest of its own texts is
 *   unspecified and nothing outside them is affected.
 *   The call has no verdict of its own: AMPH_OK or a parameter error.
 *
 *   Host mode: both tables are checked against T and out->nchars; a breach
 *   returns AMPH_E_PARAM with nothing launched.  reject[o] >= 0 rejects object
 *   o (the host form of a verdict: -1 = clean).  ONE page-locked image goes to
 *   the device (the tables, the five arrays, reject) and one comes back, copied
 *   into the caller's buffers text by text; a call that fits the small-call
 *   arena is built there and moves nothing (amph_respond_batch_copies counts).
 *
 *   AMPH_F_DEVICE: the tables and reject are 8-byte aligned device arrays, the
 *   five arrays and the five buffers 16-byte aligned (AMPH_E_PARAM otherwise);
 *   asynchronous on `stream`, behind whatever produced the verdicts there.
 *   reject[o] != AMPH_NO_FAILURE rejects object o.  The tables' contract is
 *   the CALLER's: whatever they hold, nothing outside the five arrays' T words
 *   is read and nothing outside the five buffers' nchars characters written.
 *
 *   AMPH_F_ACCUMULATE and AMPH_F_HOST_IO are refused (AMPH_E_PARAM).  A
 *   multi-device context runs these calls on devices[0].  n_objects == 0 or
 *   T == 0 returns AMPH_OK and launches nothing. */
int amph_odo_fields_b64_packed(amph_ctx* ctx, const amph_odo* fields, const uint64_t* word_offsets,
                               const uint64_t* text_offsets, size_t n_objects, const amph_odo_b64_out* out,
                               const int64_t* reject, uint32_t flags, void* stream);

/* ---- GATHER form, host memory only (any flag: AMPH_E_PARAM) ---------------------
 * odos[o]: object o's five arrays of odos[o].nbytes bytes each; not a multiple
 * of 16: AMPH_E_LEN naming the object, before any GPU work.  out_fields[5 * o +
 * k] receives field k's text of object o (amph_wire's length for nbytes / 16
 * words, no terminator).  The library gathers the words into page-locked
 * staging, runs the packed path once and scatters the 5 n_objects texts.
 * reject: NULL or n_objects host words, reject[o] >= 0 rejects. */
int amph_odo_fields_b64_batch(amph_ctx* ctx, const amph_odo* odos, size_t n_objects, char* const* out_fields,
                              const int64_t* reject, uint32_t flags);

/* Host-device copies (hipMemcpy calls) the host mode of the two calls above
 * has issued on this context so far: 2 per staged call, whatever n_objects is,
 * and 0 for a call that fits the small-call arena. */
uint64_t amph_respond_batch_copies(const amph_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* AMPHORA_RESPOND_BATCH_H_ */
