/*
 * amphora_wire_batch.h -- extension of amphora.h: K_RV / K_MASK for MANY
 * secrets straight from their base64 wire texts, in one launch, with one MAC
 * verdict and one bad-character verdict per secret.
 *
 * It joins the two forms amphora.h keeps apart: the wire-text calls
 * (amph_recombine_verify_b64 / amph_mask_input_b64: the parties' base64 JSON
 * fields decoded in LDS, one secret per call) and the many-secrets calls
 * (amph_*_packed / amph_*_batch: K secrets per launch, decoded words only).
 * A client holding K small secrets x n parties x 5 base64 strings -- K
 * getSecret / createSecret requests, DefaultAmphoraClient.java:206-217 /
 * 150-170, each with Jackson's base64 decode of every byte[] field -- gets
 * per secret exactly what the single wire-text call on that secret alone
 * gives.  Same conventions as amphora.h (status codes, flags, amph_last_error,
 * threading).  The JSON-framed output of amph_mask_input_json has no batch
 * form: each createSecret is its own POST (MaskedInput.java:25-62).
 */
#ifndef AMPHORA_WIRE_BATCH_H_
#define AMPHORA_WIRE_BATCH_H_

#include "amphora.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- PACKED form: slotted text ---------------------------------------------
 * Buffers: one per (party, field), 5 n_parties in all, as amph_odo_b64; each
 * holds EVERY object's own base64 text of that field, complete with its own
 * '=' padding, at a slot offset.  odos[j].nchars is the buffers' length, equal
 * over the parties (AMPH_E_LEN otherwise).
 *   word_offsets[n_objects + 1]: the packed calls' table (offsets[0] = 0,
 *   nondecreasing, last entry T).  Object o has W_o = word_offsets[o + 1] -
 *   word_offsets[o] words and a text of nchars_o = 4 * ceil(16 * W_o / 3)
 *   characters.
 *   text_offsets[n_objects]: the character offset of object o's text, the same
 *   in all 5 n buffers; every entry a multiple of 16 (the kernels load aligned
 *   16-byte units); slots ordered and disjoint, text_offsets[o] + nchars_o <=
 *   text_offsets[o + 1], and the last one fits: text_offsets[n_objects - 1] +
 *   nchars_(n_objects - 1) <= nchars.  Bytes between one text's end and the
 *   next slot, and after the last text, are NEVER READ: a buffer may end at
 *   the last text's last character.  amph_wire_slot_chars(words) = nchars
 *   rounded up to 16, the stride of the dense layout.
 *   Outputs: out_secrets / out_masked16 (16 T bytes) and out_records24 (24 T
 *   characters, MaskedInputData.java:44-52) are packed on word_offsets, and so
 *   are amph_mask_input_b64_packed's secrets -- one per mask word, there is no
 *   verify-only tail (as amph_mask_input_packed).  out_masked16 and / or
 *   out_records24 may be NULL.  first_fail and bad_char have n_objects entries.
 *
 *   Host mode: both tables are checked; a breach returns AMPH_E_PARAM with
 *   nothing launched.  Per object: bad_char[o] = -1 or the smallest (5 * party
 *   + field) * nchars_o + offset of a character outside the alphabet, as
 *   amph_recombine_verify_b64 counts it on that object alone.  When
 *   bad_char[o] >= 0, first_fail[o] = -1 and the object's output words are
 *   unspecified (a text that does not parse has no MAC verdict).  Otherwise
 *   first_fail[o] = -1 or the object's smallest failing word counted from its
 *   first word, and its outputs are written, failed or not.  Every object's
 *   outputs and verdicts are bit-identical to the single wire-text call on
 *   that object alone.  Status: AMPH_E_PARAM if any object has a bad
 *   character, else AMPH_E_VERIFY if any object failed its MACs, else AMPH_OK;
 *   amph_last_error names the first such object and how many there were.
 *   The texts (and secrets) move to the device as ONE page-locked image, the
 *   outputs and both verdict arrays come back as one: the number of
 *   host-device copies does not grow with n_objects
 *   (amph_wire_batch_copies counts them).
 *
 *   AMPH_F_DEVICE: the tables and the verdict arrays are device arrays, 8-byte
 *   aligned; text pointers, outputs and secrets 16-byte aligned; asynchronous
 *   on `stream`.  Both verdict arrays are reset to AMPH_NO_FAILURE unless
 *   AMPH_F_ACCUMULATE is set (then min-combined).  The tables' contract is the
 *   CALLER's: whatever they hold, nothing outside [0, n_objects) of the
 *   verdict arrays is written, and no output word past word_offsets[n_objects]
 *   (T, by the caller's word: the packed outputs hold that many words).
 *
 *   AMPH_F_HOST_IO is refused (AMPH_E_PARAM).  A multi-device context runs
 *   these calls on devices[0].  n_objects == 0 returns AMPH_OK and launches
 *   nothing; an object of 0 words reads nothing and stays clean. */
size_t amph_wire_slot_chars(size_t words);

int amph_recombine_verify_b64_packed(amph_ctx* ctx, const amph_odo_b64* odos, int n_parties,
                                     const uint64_t* word_offsets, const uint64_t* text_offsets,
                                     size_t n_objects, uint8_t* out_secrets, int64_t* first_fail,
                                     int64_t* bad_char, uint32_t flags, void* stream);
int amph_mask_input_b64_packed(amph_ctx* ctx, const amph_odo_b64* mask_odos, int n_parties,
                               const uint64_t* word_offsets, const uint64_t* text_offsets,
                               size_t n_objects, const uint8_t* secrets, uint8_t* out_masked16,
                               char* out_records24, int64_t* first_fail, int64_t* bad_char,
                               uint32_t flags, void* stream);

/* ---- GATHER form, host memory only (any flag: AMPH_E_PARAM) ------------------
 * One amph_odo_b64 per object per party, odos[o * n_parties + j] = party j's
 * five texts of object o, and one words[o] per object: odos[o * n_parties +
 * j].nchars must equal 4 * ceil(16 * words[o] / 3), else AMPH_E_LEN (the
 * message names object and party) before any GPU work.  The library gathers
 * the texts (and secrets[o], words[o] LE16 integers each) into the dense
 * slotted layout in page-locked memory, runs the packed path once and scatters
 * out_secrets[o] / out_masked16[o] / out_records24[o].  Verdicts, outputs and
 * status are the packed form's host mode.  out_masked16 and / or
 * out_records24 may be NULL (the whole array). */
int amph_recombine_verify_b64_batch(amph_ctx* ctx, const amph_odo_b64* odos, int n_parties,
                                    size_t n_objects, const size_t* words, uint8_t* const* out_secrets,
                                    int64_t* first_fail, int64_t* bad_char, uint32_t flags);
int amph_mask_input_b64_batch(amph_ctx* ctx, const amph_odo_b64* mask_odos, int n_parties,
                              size_t n_objects, const size_t* words, const uint8_t* const* secrets,
                              uint8_t* const* out_masked16, char* const* out_records24,
                              int64_t* first_fail, int64_t* bad_char, uint32_t flags);

/* Host-device copies (hipMemcpy calls) the host mode of the four calls above
 * has issued on this context so far: a constant number per call, whatever
 * n_objects is (0 for a call that fits the small-call arena, whose kernels
 * read and write page-locked memory in place). */
uint64_t amph_wire_batch_copies(const amph_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* AMPHORA_WIRE_BATCH_H_ */
