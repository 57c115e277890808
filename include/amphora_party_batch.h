/*
 * amphora_party_batch.h -- extension of amphora.h: MANY Output Delivery
 * requests of one party in ONE device-resident session.
 *
 * amph_party_* (amphora.h) keeps one request's triples, diffs and opened
 * values on the GPU from the tuples to the response's five base64 fields, and
 * reads each partner's interimValues text once.  A party that answers K
 * requests pays its launches and allocations K times.  amph_parties_* runs K
 * requests in one session: one K_ODO_PRE over the concatenation of their
 * words, K texts written into one buffer, every partner's K texts decoded in
 * one read, one open + product launch, one launch for the 5 K base64 texts.
 * The number of kernel launches does not depend on K, every request has its
 * own verdict, and per request every result is bit for bit what an
 * amph_party_* session gives on that request alone.  Same conventions as
 * amphora.h (status codes, amph_last_error, threading: one call at a time per
 * session); AMPH_F_HOST_IO has no meaning here (the calls take no flags).
 *
 * A caller with ONE large request keeps amph_party_*: this form lays the
 * texts out by their longest possible length, runs the encode's own length
 * pass and looks every tile's object up -- measured on an MI355X, three
 * parties, device mode, 4 Mi words in total: 1.72 against 1.35 ms for one
 * request, 2.0 against 6.1 ms for 64, 2.4 against 76.6 ms for 1,024
 * (DESIGN.md 4c-next).
 *
 * LAYOUT.  word_offsets[n_objects + 1] (host memory in both modes; the session
 * keeps a copy): 0 first, nondecreasing, T = the total last; object o holds
 * words [word_offsets[o], word_offsets[o + 1]) of every packed array -- share
 * data (stride 16 or 32), 2 T mask tuples of 32 bytes, 2 T triples of 96, and
 * the five fields of 16 T bytes -- and pairs 2 * word_offsets.  An object of 0
 * words is legal: its text is "[]", its five fields are empty.
 *   Texts: ONE buffer of amph_parties_text_bytes characters in the dense
 * layout of amphora_exchange_batch.h, text_offsets[o] = the sum of
 * amph_exchange_slot_chars(P_i) over i < o.  It depends on the word counts
 * alone, so every party of the exchange has the same layout, and a partner's
 * buffer goes into amph_parties_partner(_dev) unchanged.  Bytes outside the
 * texts are never written by a device-mode session; a host-mode session's
 * buffer holds 0 there.
 *   Fields: five buffers of amph_parties_field_chars characters in the dense
 * layout of amphora_respond_batch.h / amphora_wire_batch.h, field_offsets[o] =
 * the sum of amph_wire_slot_chars(W_i) over i < o:
 * amph_recombine_verify_b64_packed reads them unchanged.
 *
 * DEVICE MEMORY, per word of T (a word = 2 pairs = 4 exchange values):
 *   session: 5 x 16 (fields) + 64 + 4 (this party's diffs) + 184 (its texts,
 *   at most: 92 per pair) + 5 x 21.4 (base64) = about 440 bytes, plus 192 for
 *   the triples in host mode and the staged share data and masks during
 *   begin;
 *   per partner: the span form, 17 bytes per slot and 528 slots per 8 KiB of
 *   text buffer = about 202 bytes, plus 4 x 17 = 68 bytes of pair-order rows
 *   (the rows of an object whose text is not Jackson's compact output: it
 *   alone falls back to them), plus 16 bytes per 64 words of windows; host
 *   mode stages the partner's texts (184 bytes) once for all slots.
 * Buffers come from and return to the context's pool as amph_party's do.
 *
 * STREAMS (the _dev calls).  Every call only ENQUEUES on `stream` and returns;
 * amph_parties_free is the one call that waits (for the session's latest
 * stream).  The word_offsets table is uploaded asynchronously from page-locked
 * memory the session owns.  amph_parties_partner_dev reports into the caller's
 * bad_index on `stream`, copies the K verdict words into the session and
 * records an event: the caller's array is free once `stream` has passed the
 * call, and amph_parties_finish_b64_dev -- on any stream -- waits for every
 * accepted partner call's event.  The caller's tuples, triples and optional
 * y / r / v buffers are used in place until the finish call's work is done.
 */
#ifndef AMPHORA_PARTY_BATCH_H_
#define AMPHORA_PARTY_BATCH_H_

#include "amphora.h"
#include "amphora_exchange_batch.h"
#include "amphora_respond_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct amph_parties amph_parties;

/* `object` of amph_parties_text: the whole text buffer */
#define AMPH_PARTIES_ALL ((size_t)-1)

/* K_ODO_PRE over the T words, then the K texts (launches: one plus the
 * segmented encode's four).  out_y / out_r / out_v: NULL or 16 T bytes each
 * (device mode: 16-byte aligned device buffers the fields then live in).
 * n_objects == 0, a table that is not 0-first and nondecreasing, share_stride
 * other than 16 / 32 or n_parties outside [1, 16]: AMPH_E_PARAM before any
 * GPU work.  A multi-device context runs host sessions on its first device
 * and refuses device mode. */
int amph_parties_begin(amph_ctx* ctx, const uint8_t* share_data, size_t share_stride, const uint8_t* masks,
                       const uint8_t* triples, const uint64_t* word_offsets, size_t n_objects, int n_parties,
                       uint8_t* out_y, uint8_t* out_r, uint8_t* out_v, amph_parties** out);
int amph_parties_begin_dev(amph_ctx* ctx, const uint8_t* share_data, size_t share_stride, const uint8_t* masks,
                           const uint8_t* triples, const uint64_t* word_offsets, size_t n_objects, int n_parties,
                           uint8_t* out_y, uint8_t* out_r, uint8_t* out_v, void* stream, amph_parties** out);

size_t amph_parties_objects(const amph_parties* p);
size_t amph_parties_words(const amph_parties* p);       /* T */
size_t amph_parties_text_bytes(const amph_parties* p);  /* the text buffer */
size_t amph_parties_field_chars(const amph_parties* p); /* each field buffer */
/* the n_objects offsets of the texts / of the field texts */
int amph_parties_text_offsets(const amph_parties* p, uint64_t* out);
int amph_parties_field_offsets(const amph_parties* p, uint64_t* out);

/* Host mode: the n_objects text lengths; one object's text (out_cap at least
 * its length) or, with AMPH_PARTIES_ALL, the whole buffer (out_cap at least
 * amph_parties_text_bytes). */
int amph_parties_text_lens(amph_parties* p, uint64_t* out);
int amph_parties_text(amph_parties* p, size_t object, char* out, size_t out_cap);
/* Device mode: the device addresses of the buffer, its offsets table and the
 * lengths the encode wrote (valid until amph_parties_free; the lengths once
 * the begin call's stream has run). */
int amph_parties_text_dev(amph_parties* p, const char** texts, const uint64_t** text_offsets,
                          const uint64_t** text_lens);

/* One partner's K texts into slot 1 .. n_parties - 1: ONE buffer with object
 * o's text at the session's text_offsets[o], text_lens[o] characters long
 * (launches: the span pass, the scan's two, the checks / windows / general
 * pass).  Per object bad_index[o] is amph_exchange_decode_packed's: -1
 * (AMPH_NO_FAILURE in device mode) when clean, the offending byte's offset
 * inside the object's own text, or text_lens[o] when the text is well-formed
 * but does not hold P_o pairs.  A faulty, whitespace-bearing or small-valued
 * text may cost its neighbours time, never a byte or a verdict.
 *   Host mode: text_lens / bad_index are host arrays of n_objects entries; a
 * length beyond its slot returns AMPH_E_PARAM before any GPU work.  Status:
 * AMPH_E_PARAM if any text was refused, AMPH_E_LEN if the only failures are
 * count mismatches; amph_last_error names the first such object.
 *   Device mode: texts 16-byte aligned, text_lens / bad_index 8-byte aligned
 * device arrays (AMPH_E_PARAM otherwise); lengths are the caller's contract:
 * whatever they hold, nothing outside the buffer's amph_parties_text_bytes
 * characters is read.
 * The slot counts as filled either way; the session min-combines the accepted
 * calls' verdicts per object at finish.  amph_parties_reset_partner frees a
 * slot (and forgets its verdicts) for a resubmission of all K texts. */
int amph_parties_partner(amph_parties* p, int slot, const char* texts, const uint64_t* text_lens,
                         int64_t* bad_index);
int amph_parties_partner_dev(amph_parties* p, int slot, const char* texts, const uint64_t* text_lens,
                             int64_t* bad_index, void* stream);
int amph_parties_reset_partner(amph_parties* p, int slot);

/* The summed diffs -> w, u for all K objects (one launch), refused while a
 * partner slot is unfilled; a session finishes once.
 *   amph_parties_finish: out_w / out_u, 16 T bytes each, packed (host mode).
 *   amph_parties_finish_b64(_dev): then ONE more launch writes the five
 * fields' K texts.  An object with any refused partner text gets "!!!!" as
 * the first four characters of its five texts; every other object's texts are
 * unaffected.  Host mode: fields_b64[k] receives amph_parties_field_chars
 * characters (0 outside the texts), rejected (NULL or n_objects bytes) 0 / 1
 * per object.  Device mode: *fields_b64[k] = the session's buffers. */
int amph_parties_finish(amph_parties* p, int is_player0, uint8_t* out_w, uint8_t* out_u);
int amph_parties_finish_b64(amph_parties* p, int is_player0, char* const fields_b64[5], uint8_t* rejected);
int amph_parties_finish_b64_dev(amph_parties* p, int is_player0, const char* fields_b64[5], void* stream);

void amph_parties_free(amph_parties* p);

#ifdef __cplusplus
}
#endif
#endif /* AMPHORA_PARTY_BATCH_H_ */
