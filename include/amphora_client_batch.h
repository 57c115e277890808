/*
 * amphora_client_batch.h -- extension of amphora.h: the CLIENT side as a
 * session for K SECRETS, one launch per party and a verdict per secret.
 *
 * amph_client_* (amphora_client_session.h) takes ONE secret's texts party by
 * party.  A client that fetches K small secrets pays K x (n + 1) launches
 * and, in host mode, K x (n + 1) synchronisations and K pool round trips.
 * amph_clients_* runs the K secrets in one session: a party's K responses
 * arrive as five slotted field buffers -- the dense layout of
 * amphora_wire_batch.h, which amph_parties_finish_b64(_dev) writes -- and are
 * added into running sums packed on word_offsets in ONE launch, whatever K
 * is; the finish calls run K_RV / K_MASK from the sums in one launch and give
 * every object its own verdicts.  Per object, outputs and verdicts are bit
 * for bit what amph_recombine_verify_b64_packed, amph_mask_input_b64_packed
 * and amph_mask_input_json_packed give on all parties' buffers at once, and
 * host-mode status and amph_last_error are theirs.  Same conventions as
 * amphora.h (status codes, amph_last_error); AMPH_F_HOST_IO has no meaning
 * here (the calls take no flags).
 *
 * WHO KEEPS WHICH CALL.  Per word the session moves 5 x (21.3 + 16 + 16)
 * bytes per party plus 96 at finish, against 106.7 per party plus 16 for the
 * packed call: about 2.5 times the HBM bytes at three parties.  A caller that
 * already holds all parties' buffers on the device keeps the packed calls.
 * The session is for responses that arrive over time: every party but the
 * last is uploaded and decoded behind the wait for the slowest, and what
 * remains after the last arrival is one party's launch and the finish.
 *   Measured on an MI355X, three parties, 4 Mi words in total, medians of 20
 * (DESIGN.md 4e).  Host mode, pageable texts: the tail after the last arrival
 * is 26.9 ms against 72.9 ms for amph_recombine_verify_b64_packed at 1,024
 * secrets (0.37; 0.44 for the mask-to-JSON finish); the whole session takes
 * 73.7 ms against 168.1 ms for a loop of 1,024 amph_client_* sessions, but
 * 72.9 against 48.7 ms for a loop of 64 and 72.2 against 25.9 ms for ONE:
 * the page-locked image costs a host copy of every text, so a caller with
 * few large secrets in host memory keeps amph_client_*.  Device mode, texts
 * resident: 0.735 ms against 62.8 ms for the loop of 1,024 and 4.9 ms for the
 * loop of 64, against 0.28 ms for the packed call; at ONE secret 0.714
 * against 0.677 ms, the segmented accumulate kernel 5 % over the one-secret
 * kernel (it looks every tile's object up).
 *
 * LAYOUT.  word_offsets[n_objects + 1] (host memory in both modes; the
 * session keeps a copy): 0 first, nondecreasing, T = the total last; object o
 * holds words [word_offsets[o], word_offsets[o + 1]) of the sums, the secrets
 * and every packed output.  An object of 0 words is legal anywhere.
 *   Texts: five buffers per party in the dense layout of
 * amphora_wire_batch.h, object o's own base64 text (its '=' padding included)
 * at field_offsets[o] = the sum of amph_wire_slot_chars(W_i) over i < o.  The
 * layout depends on the word counts alone: amph_clients_field_offsets equals
 * amph_parties_field_offsets for the same table, and a party session's
 * buffers go into amph_clients_party(_dev) unchanged.  texts->nchars may be
 * anything from the end of the last text up to amph_clients_field_chars;
 * bytes between texts and after the last text are never read.
 *   Secrets: one per mask word, packed on word_offsets (no verify-only tail,
 * as in amph_mask_input_b64_packed).
 *   Framed output: ONE buffer of amph_clients_upload_chars characters in the
 * dense layout of amphora_upload_batch.h, object o's "data" array text at
 * upload_offsets[o] = the sum of amph_upload_slot_chars(W_i) over i < o, "[]"
 * for an object of no words; amph_convert_share_json_packed reads it
 * unchanged.  Nothing outside the texts is written.
 *
 * VERDICTS.  first_fails[o]: object o's smallest failing word, counted from
 * its own first word.  bad_chars[o]: the smallest (5 party + field) *
 * nchars_o + offset over the parties, nchars_o the length of object o's own
 * text.  Host mode: -1 when clean; device mode: AMPH_NO_FAILURE.  A bad
 * character in one object never costs a neighbour a byte or a verdict and
 * does not stop the session: later parties are still accumulated and the
 * finish calls always launch (the other objects need their results).  It
 * takes precedence over that object's MAC verdict; the object's outputs are
 * unspecified.  Host-mode status: AMPH_E_PARAM if any object holds an
 * illegal character, else AMPH_E_VERIFY if any failed, with the packed
 * calls' "object N ... (k of K objects ...)" messages; the outputs of the
 * other objects are written either way.
 *
 * DEVICE MEMORY: 80 bytes per word of sums, 24 bytes per object of tables
 * (device mode: 40 more, the starts of amphora_client_bodies.h's calls) and
 * one verdict word per object, in ONE buffer taken from the context's
 * pool of party-session buffers and handed back by amph_clients_free.  Host
 * mode moves a party's K texts of the five buffers as ONE page-locked image
 * and the finish call's secrets and outputs as one image each, through the
 * context's small-call arena or its wire staging buffer: the copies per call
 * do not depend on K and are counted in amph_clients_copies.
 *
 * SLOTS.  `party` is 0 .. n_parties - 1 in any order, each slot once.  A
 * session finishes once; amph_clients_word is valid from the moment all
 * parties are in until amph_clients_free.
 *
 * THREADS.  Host-mode calls are serialised by the context's mutex: n threads
 * may each hand in their own slot.  Finish and free belong to one thread,
 * after the party calls have returned.
 *
 * STREAMS (the _dev calls).  Every call only ENQUEUES on `stream` and
 * returns; all calls of one session use ONE stream (the accumulation is a
 * read-modify-write on the sums, in stream order).  The word table is
 * uploaded asynchronously from page-locked memory the session owns.  Texts,
 * secrets, out_secrets, out_masked16 and out_text are device memory aligned
 * to 16 bytes, out_records24 and the verdict arrays to 8.  A device-mode
 * finish copies the session's K bad-character words into the caller's array
 * device to device; that copy is the one operation besides the launch.
 * amph_clients_free is the one call that waits (for the stream).  A
 * multi-device context runs host sessions on its first device and refuses
 * device mode.
 *
 * OUT OF SCOPE: ragged parties (every party answers every object); a slot
 * handed in twice (resubmission); a fused "last party + finish" launch;
 * caller-chosen text offsets in THESE calls (the slotted layout is fixed;
 * amphora_client_bodies.h hands the same session a party's response bodies
 * as they lie, every text at its own byte); the C++ mirror, JNI and Java
 * bindings (none of the many-objects headers has them).
 */
#ifndef AMPHORA_CLIENT_BATCH_H_
#define AMPHORA_CLIENT_BATCH_H_

#include "amphora.h"
#include "amphora_upload_batch.h"
#include "amphora_wire_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct amph_clients amph_clients;

/* The sums, zeroed on the session's stream.  n_objects == 0, a table that is
 * not 0-first and nondecreasing or n_parties outside [1, 16]: AMPH_E_PARAM
 * before any GPU work. */
int amph_clients_begin(amph_ctx* ctx, const uint64_t* word_offsets, size_t n_objects, int n_parties,
                       amph_clients** out);

size_t amph_clients_objects(const amph_clients* s);
size_t amph_clients_words(const amph_clients* s); /* T */
int amph_clients_parties_seen(const amph_clients* s);
size_t amph_clients_field_chars(const amph_clients* s);  /* each slotted field buffer */
size_t amph_clients_upload_chars(const amph_clients* s); /* the framed output buffer */
/* the n_objects offsets of the field texts / of the framed texts */
int amph_clients_field_offsets(const amph_clients* s, uint64_t* out);
int amph_clients_upload_offsets(const amph_clients* s, uint64_t* out);

/* One party's five slotted buffers into its slot: ONE launch whatever
 * n_objects is.  texts->nchars below the end of the last text: AMPH_E_LEN,
 * nothing is launched and the slot stays open.  A slot already taken, or
 * outside [0, n_parties): AMPH_E_PARAM, nothing is launched.  bad_chars (NULL
 * or n_objects entries): this call's verdict per object.  Host mode waits
 * and returns AMPH_E_PARAM with the packed calls' message when any object
 * holds an illegal character; the slot counts as taken either way. */
int amph_clients_party(amph_clients* s, int party, const amph_odo_b64* texts, int64_t* bad_chars);

/* amph_recombine_verify_b64_packed from the sums (one launch): out_secrets,
 * 16 T bytes packed on word_offsets.  A slot still open: AMPH_E_PARAM naming
 * it (the session stays usable).  first_fails / bad_chars: n_objects entries
 * each, both required. */
int amph_clients_finish_verify(amph_clients* s, uint8_t* out_secrets, int64_t* first_fails, int64_t* bad_chars);

/* amph_mask_input_b64_packed from the sums (one launch): secrets 16 T bytes,
 * out_masked16 (16 T bytes) and / or out_records24 (24 T characters), either
 * may be NULL. */
int amph_clients_finish_mask(amph_clients* s, const uint8_t* secrets, uint8_t* out_masked16, char* out_records24,
                             int64_t* first_fails, int64_t* bad_chars);

/* amph_mask_input_json_packed from the sums (one launch): out_text in the
 * dense upload layout; out_cap below amph_clients_upload_chars: AMPH_E_LEN. */
int amph_clients_finish_mask_json(amph_clients* s, const uint8_t* secrets, char* out_text, size_t out_cap,
                                  int64_t* first_fails, int64_t* bad_chars);

/* The five recombined values of word `index` of object `object` as canonical
 * little-endian integers, in ODO order y, r, v, w, u.  Waits for the
 * session's stream.  AMPH_E_PARAM while a slot is open, AMPH_E_RANGE for an
 * object or an index out of range. */
int amph_clients_word(amph_clients* s, size_t object, size_t index, uint8_t out_yrvwu[5][16]);

/* hipMemcpy calls of the host-mode calls of this header so far (0 for every
 * call that fits the small-call arena); amph_wire_batch_copies keeps its
 * meaning and does not count them. */
uint64_t amph_clients_copies(const amph_ctx* ctx);

void amph_clients_free(amph_clients* s);

/* Device mode: the same calls on device memory, asynchronous on `stream`. */
int amph_clients_begin_dev(amph_ctx* ctx, const uint64_t* word_offsets, size_t n_objects, int n_parties,
                           void* stream, amph_clients** out);
int amph_clients_party_dev(amph_clients* s, int party, const amph_odo_b64* texts, int64_t* bad_chars, void* stream);
int amph_clients_finish_verify_dev(amph_clients* s, uint8_t* out_secrets, int64_t* first_fails, int64_t* bad_chars,
                                   void* stream);
int amph_clients_finish_mask_dev(amph_clients* s, const uint8_t* secrets, uint8_t* out_masked16,
                                 char* out_records24, int64_t* first_fails, int64_t* bad_chars, void* stream);
int amph_clients_finish_mask_json_dev(amph_clients* s, const uint8_t* secrets, char* out_text, size_t out_cap,
                                      int64_t* first_fails, int64_t* bad_chars, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AMPHORA_CLIENT_BATCH_H_ */
