/*
 * amphora_client_session.h -- extension of amphora.h: the CLIENT side as a
 * session that takes each party's response text as it arrives.
 *
 * amph_recombine_verify_b64, amph_mask_input_b64 and amph_mask_input_json
 * (amphora.h) need all n parties' five base64 texts before anything starts:
 * in host mode the 5 n texts are uploaded after the slowest party has
 * answered, and the device holds 107 n bytes of text per word at once.  A
 * client receives the responses one by one (the reference fans out over the
 * parties in parallel).  Recombination is a sum mod p of canonical Montgomery
 * words, exact in any order, so a session adds each party's five texts into
 * five running sums on the device the moment they arrive
 * (amph_client_party: ONE launch, the decoded words never reach HBM) and
 * finishes from the sums alone -- secrets, verdicts, masked words, records
 * and the framed MaskedInput "data" text bit for bit what the whole calls
 * give on the same texts.  Same conventions as amphora.h (status codes,
 * amph_last_error); AMPH_F_HOST_IO has no meaning here (the calls take no
 * flags).
 *
 * WHAT IT COSTS.  Per word the session moves 5 x (21.3 + 16 + 16) bytes per
 * party (text in, sums read and written) plus 96 at finish, against 106.7 per
 * party plus 16 for the whole call: about 2.5 times the HBM bytes, and n + 1
 * launches (host mode: n + 1 synchronisations) instead of one.  A caller that
 * already holds all texts on the device keeps amph_recombine_verify_b64; the
 * session is for texts that arrive over time -- the upload and decode of
 * every party but the last hide behind the wait for the slowest -- and for
 * bounding device memory at many parties (DESIGN.md 4d has the measurements).
 *
 * DEVICE MEMORY: 80 bytes per word of sums (five fields of 16 bytes) and two
 * verdict words, in ONE buffer taken from the context's pool of party-session
 * buffers (amph_party's pool) and handed back to it by amph_client_free; host
 * mode also stages one party's five texts (107 bytes per word), the finish
 * call's secrets and its outputs in the context's staging buffer of the wire-text
 * calls (or its small-call arena), which is shared with them, not owned.
 *
 * SLOTS.  `party` is 0 .. n_parties - 1 in any order, each slot once.  All
 * parties' texts have the one length that `words` words code to: nchars =
 * 4 ceil(16 words / 3).  A session finishes once; amph_client_word is valid
 * from the moment all parties are in until amph_client_free.
 *
 * BAD CHARACTERS are reported with the whole call's encoding, (5 party +
 * field) * nchars + offset.  A bad character does not stop the session: later
 * parties are still accumulated, the session keeps the minimum over all
 * parties, and the finish calls return AMPH_E_PARAM with it and the whole
 * call's message.  It takes precedence over AMPH_E_VERIFY.  Host mode writes
 * no output on either error.
 *
 * THREADS.  Host-mode calls are serialised by the context's mutex: n threads
 * may each hand in their own slot concurrently.  Finish and free belong to
 * one thread, after the party calls have returned.
 *
 * STREAMS (the _dev calls).  Every call only enqueues on `stream` and
 * returns; all calls of one session use ONE stream (the accumulation is a
 * read-modify-write on the sums, in stream order).  Texts, secrets, outputs
 * and verdict words are device memory aligned as the whole calls': texts,
 * secrets, out_secrets, out_masked16 and out_text to 16 bytes, out_records24
 * and the verdict words to 8.  The verdict words are written on the stream
 * (AMPH_NO_FAILURE when clean); outputs are unspecified when bad_char is set.
 * amph_client_free is the one call that waits (for the stream).  A
 * multi-device context runs host sessions on its first device and refuses
 * device mode.
 */
#ifndef AMPHORA_CLIENT_SESSION_H_
#define AMPHORA_CLIENT_SESSION_H_

#include "amphora.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct amph_client amph_client;

/* The sums, zeroed on the session's stream.  words == 0 is valid: every call
 * of the session then returns AMPH_OK and launches nothing.  n_parties outside
 * [1, 16]: AMPH_E_PARAM. */
int amph_client_begin(amph_ctx* ctx, size_t words, int n_parties, amph_client** out);

/* One party's five texts into its slot: ONE launch.  texts->nchars other than
 * 4 ceil(16 words / 3): AMPH_E_LEN, nothing is launched and the slot stays
 * open.  A slot already taken, or outside [0, n_parties): AMPH_E_PARAM,
 * nothing is launched.  Host mode waits and returns this party's verdict:
 * *bad_char = -1, or the smallest offending character and AMPH_E_PARAM with
 * the whole call's message; the slot counts as taken either way. */
int amph_client_party(amph_client* s, int party, const amph_odo_b64* texts, int64_t* bad_char);

/* amph_recombine_verify_b64 from the sums (one launch): out_secrets, 16 words
 * bytes.  A slot still open: AMPH_E_PARAM naming it (the session stays
 * usable). */
int amph_client_finish_verify(amph_client* s, uint8_t* out_secrets, int64_t* first_fail, int64_t* bad_char);

/* amph_mask_input_b64 from the sums (one launch): out_masked16 (16 n_secrets
 * bytes) and / or out_records24 (24 n_secrets characters), either may be
 * NULL; every mask is verified whatever n_secrets is.  n_secrets > words:
 * the masks are verified first, then AMPH_E_LEN. */
int amph_client_finish_mask(amph_client* s, const uint8_t* secrets, size_t n_secrets, uint8_t* out_masked16,
                            char* out_records24, int64_t* first_fail, int64_t* bad_char);

/* amph_mask_input_json from the sums (one launch): out_text receives
 * amph_masked_input_data_chars(n_secrets) characters; out_cap below that:
 * AMPH_E_LEN. */
int amph_client_finish_mask_json(amph_client* s, const uint8_t* secrets, size_t n_secrets, char* out_text,
                                 size_t out_cap, int64_t* first_fail, int64_t* bad_char);

/* The five recombined values of word `index` as canonical little-endian
 * integers, in ODO order y, r, v, w, u (what a failure message is rendered
 * from: the session no longer holds the parties' texts).  Waits for the
 * session's stream.  AMPH_E_PARAM while a slot is open, AMPH_E_RANGE for
 * index >= words. */
int amph_client_word(amph_client* s, size_t index, uint8_t out_yrvwu[5][16]);

size_t amph_client_words(const amph_client* s);
int amph_client_parties_seen(const amph_client* s);
void amph_client_free(amph_client* s);

/* Device mode: the same calls on device memory, asynchronous on `stream`. */
int amph_client_begin_dev(amph_ctx* ctx, size_t words, int n_parties, void* stream, amph_client** out);
int amph_client_party_dev(amph_client* s, int party, const amph_odo_b64* texts, int64_t* bad_char, void* stream);
int amph_client_finish_verify_dev(amph_client* s, uint8_t* out_secrets, int64_t* first_fail, int64_t* bad_char,
                                  void* stream);
int amph_client_finish_mask_dev(amph_client* s, const uint8_t* secrets, size_t n_secrets, uint8_t* out_masked16,
                                char* out_records24, int64_t* first_fail, int64_t* bad_char, void* stream);
int amph_client_finish_mask_json_dev(amph_client* s, const uint8_t* secrets, size_t n_secrets, char* out_text,
                                     size_t out_cap, int64_t* first_fail, int64_t* bad_char, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AMPHORA_CLIENT_SESSION_H_ */
