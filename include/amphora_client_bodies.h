/*
 * amphora_client_bodies.h -- extension of amphora_client_batch.h: a party's
 * K answers handed to the K-secret client session AS THE RESPONSE BODIES LIE
 * in memory.
 *
 * amph_clients_party takes a party's K answers as five slotted field buffers
 * with every text moved to a multiple of 16.  A client holds K HTTP response
 * bodies instead, the five base64 members somewhere inside each.  The calls
 * here work on an amph_clients session (amph_clients_begin / _begin_dev) and
 * fill a party's slot from the bodies: amph_bodies_scan finds the five
 * members of one body on the host, and amph_bodies_party(_dev) decodes every
 * member at whatever byte offset it has -- still ONE launch per party
 * whatever K is.  Sums, verdict words, the finish calls and every rule of
 * amphora_client_batch.h (slots, threads, streams, verdict encoding) are that
 * header's; a session may take some parties through amph_clients_party and
 * others through these calls.
 *
 * CONTRACT: WHICH BYTES ARE READ.  The device sees the bodies in one 16-byte
 * aligned buffer.  Cut it into aligned granules of 16 bytes.  Of a text of
 * nchars characters at byte `start`, the kernel reads bytes of the granules
 * start / 16 .. (start + nchars - 1) / 16 only -- those that hold at least one
 * of its characters -- and interprets only the text's own bytes.  As built
 * (AMPH_BODY_FETCH = 1) every 16-character unit is ONE 16-byte load at the
 * text's own alignment: exactly the text's bytes are read.  Built with
 * -DAMPH_BODY_FETCH=0 a unit is funnelled out of the one or two whole granules
 * that hold it: up to 15 bytes in front of a text and up to 15 behind it are
 * then LOADED but never interpreted.  Either way, whatever lies around a text
 * -- JSON, a neighbouring member, 0xFF -- changes no output and no verdict; the
 * characters of a text's last units (the tile that holds the '=' padding) are
 * read one by one; no granule without text is read and nothing is written to
 * the buffer.  In device mode the buffer's allocation must reach the next
 * multiple of 16 past its last text (the granule form relies on it); in host
 * mode the library lays the bodies out itself.  An object of 0 words reads
 * nothing.
 *
 * ABSENT OBJECTS.  A start of AMPH_BODY_ABSENT in any of an object's five
 * entries marks the object absent for this party (its body was malformed, or
 * its texts have another length than the session's word table says).  Nothing
 * of it is read; the object's verdict word takes (5 party) * nchars_o -- an
 * illegal character at index 0 of the party's secretShares, exactly what a
 * slot of NUL bytes reports through amph_clients_party -- nothing is added to
 * its sums, and its neighbours keep their bytes and verdicts.
 *
 * WHO KEEPS WHICH CALL.  Measured on an MI355X, three parties, 4 Mi words in
 * total as K = 1 / 64 / 1,024 objects, medians of 20, the forms alternating
 * in one process ("The bodies where they lie").
 *   Device mode, texts resident, the three party launches of a session:
 * 0.646 / 0.646 / 0.670 ms through amph_bodies_party_dev against 0.598 /
 * 0.591 / 0.586 ms through amph_clients_party_dev on slotted buffers, 1.08 -
 * 1.14: the any-alignment fetch costs the kernel more than the slotted fetch
 * (the granule form, AMPH_BODY_FETCH = 0, costs more still: 0.737 / 0.746 /
 * 0.829 ms, its kernel 239 - 258 us against 192 - 193 us).  A caller whose
 * texts ARE already slotted on the device -- the buffers
 * amph_parties_finish_b64_dev writes -- keeps amph_clients_party_dev; a caller
 * that received bodies into device memory uses this call and skips a gather
 * kernel of its own.
 *   Host mode, pageable memory, the three party calls: 72.2 / 73.5 / 70.7 ms
 * through amph_bodies_party against 70.7 / 72.5 / 70.2 ms through
 * amph_clients_party on buffers that were gathered BEFORE the clock started,
 * 1.01 - 1.02: the call itself is no faster -- both copy every text once into
 * the page-locked image, one memcpy per body against 5 K per party, and the
 * image holds the JSON framing too.  What these calls remove is the gather in
 * front of amph_clients_party, which the C and JNI callers had no code for and
 * which costs the Python layer more than the call: ResponseSessions.add_bodies
 * for all three parties takes 434 / 418 / 428 ms in place against 900 / 619 /
 * 623 ms with wire.odo_field_texts and the gather (0.48 / 0.67 / 0.69).  A
 * caller that holds response bodies uses these calls; a caller that holds
 * slotted buffers keeps amph_clients_party.  The 72 ms of the page-locked
 * layout against 26 ms for the one-secret session (amphora_client_batch.h)
 * stand as they were: this header removes the gather, not the image.
 *
 * OUT OF SCOPE: the one-secret session (amph_client_*: its caller holds one
 * body and pays one gather); the packed whole calls (all parties at once:
 * amphora_wire_batch.h); a GPU-side scanner (the scan is host code, a few
 * passes of memchr per body); the JNI and C++ mirrors.
 */
#ifndef AMPHORA_CLIENT_BODIES_H_
#define AMPHORA_CLIENT_BODIES_H_

#include "amphora_client_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AMPH_BODY_ABSENT UINT64_MAX

/* The five top-level members of ONE body in ODO order (secretShares, rShares,
 * vShares, wShares, uShares): starts[k] = the byte of `body` where member k's
 * base64 text begins (after its opening quote), lens[k] = its characters.
 * Pure host code, no context.  Only the PLAIN form is accepted: an enclosing
 * object, each member once, a string, no backslash in it.  Anything else --
 * a member missing, null, not a string or given twice, an escape inside a
 * value, an unterminated string, no enclosing object -- is AMPH_E_PARAM with
 * the reason in amph_last_error and nothing written; the caller then parses
 * the body its own way.  Nested keys of the same names (a tag whose key or
 * value is "rShares") are not members.  Nothing outside [body, body + len)
 * is read. */
int amph_bodies_scan(const char* body, size_t len, uint64_t starts[5], uint64_t lens[5]);

/* Host mode: party `party`'s K bodies into its slot, ONE launch.  bodies[o] /
 * body_lens[o]: object o's body; starts: K x 5 entries, starts[5 o + k] the
 * byte of bodies[o] where field k's text begins (as amph_bodies_scan gives
 * it), or AMPH_BODY_ABSENT.  Object o's texts have the nchars_o characters
 * the session's word table fixes (amph_wire_text_chars of its words).  Every
 * present body is copied whole, once, to a multiple of 16 of the call's
 * page-locked image; host-device copies per call are amph_clients_party's
 * (none in the small-call arena, two when staged) and are counted in
 * amph_clients_copies.  A start with start + nchars_o past its body, a null
 * body of a present object, a slot taken or out of range: AMPH_E_PARAM before
 * any GPU work, the slot stays open.  The call waits and returns the status
 * alone: AMPH_E_PARAM with the packed calls' "object N ..." message in
 * amph_last_error when any object holds an illegal character (an absent
 * object does); the slot counts as taken either way.  The per-object
 * verdicts are the session's and come out of the finish calls. */
int amph_bodies_party(amph_clients* s, int party, const char* const* bodies, const size_t* body_lens,
                      const uint64_t* starts);

/* Device mode: `buffer` is device memory of `nbytes` bytes that holds the K
 * bodies (or just their texts) anywhere, 16-byte aligned, its allocation
 * reaching the next multiple of 16 past nbytes.  starts: K x 5 entries in
 * HOST memory, absolute bytes of `buffer`, or AMPH_BODY_ABSENT; the call
 * copies them into page-locked memory the session owns -- one table per party
 * slot, so a later call never overwrites a table still in flight -- and
 * uploads that asynchronously; the caller's array is free on return.  The
 * call only ENQUEUES on `stream` (the session's one stream).  A start with
 * start + nchars_o past nbytes, a misaligned buffer or a slot taken:
 * AMPH_E_PARAM, nothing is enqueued. */
int amph_bodies_party_dev(amph_clients* s, int party, const char* buffer, size_t nbytes, const uint64_t* starts,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AMPHORA_CLIENT_BODIES_H_ */
