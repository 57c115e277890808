/*
 * amphora_exchange_batch.h -- extension of amphora.h: the Beaver exchange
 * texts of MANY requests written and parsed per call.
 *
 * A party that answers K Output Delivery requests runs ONE amph_odo_pre and
 * ONE amph_open_post over the concatenation of their words
 * (amphora_respond_batch.h), but between them every request exchanges its own
 * MultiplicationExchangeObject with every partner: K interimValues texts out,
 * K (n - 1) in.  amph_exchange_encode / amph_exchange_decode take one text per
 * call.  The calls here take K: a packed form (host or device memory) and a
 * gather form (host), a fixed number of kernel launches whatever K is, and one
 * verdict per object.  Per object the result is the single call's on that
 * object alone.  Same conventions as amphora.h (status codes, flags,
 * amph_last_error, threading).
 *
 * Diffs use amph_odo_pre's layout throughout: mag16 holds two LE16 magnitudes
 * per pair (d, then e), neg two sign bytes per pair.
 */
#ifndef AMPHORA_EXCHANGE_BATCH_H_
#define AMPHORA_EXCHANGE_BATCH_H_

#include "amphora.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Every text starts on a multiple of this in its buffer: the span of text one
 * parse workgroup reads, so every workgroup reads one object's text. */
#define AMPH_EXCHANGE_SLOT_ALIGN 8192

/* The dense layout's stride: amph_exchange_max_chars(npairs) rounded up to
 * AMPH_EXCHANGE_SLOT_ALIGN. */
size_t amph_exchange_slot_chars(size_t npairs);

/* ---- PACKED form ----------------------------------------------------------------
 *   mag16 / neg: the concatenation of the objects' diffs, npairs_total pairs.
 *   pair_offsets[n_objects + 1]: object o holds pairs [pair_offsets[o],
 *   pair_offsets[o + 1]), P_o of them; pair_offsets[0] = 0, nondecreasing, the
 *   last entry npairs_total.
 *   text_offsets[n_objects]: object o's text starts text_offsets[o] characters
 *   into the ONE text buffer; every entry a multiple of
 *   AMPH_EXCHANGE_SLOT_ALIGN, strictly increasing, the slots disjoint.
 *     encode: slot o holds at least amph_exchange_max_chars(P_o) characters
 *     before the next slot and before out_cap.
 *     decode: text_lens[o] characters at text_offsets[o] end at or before
 *     texts_len and before the next slot.
 *   The encode's out, text_offsets and out_lens ARE the decode's texts,
 *   text_offsets and text_lens: a partner's buffer needs no repacking.
 *
 *   Encode, per object: the text is byte-identical to amph_exchange_encode of
 *   that object's diffs (Jackson's compact output; "[]" for 0 pairs) and
 *   out_lens[o] its length.  Bytes of out outside the n_objects texts -- the
 *   rest of every slot, the gaps, everything behind the last text -- are NEVER
 *   WRITTEN.
 *
 *   Decode, per object: mag16, neg and bad_index[o] are those of
 *   amph_exchange_decode(text_o, text_lens[o], P_o): bad_index[o] = -1 when
 *   clean (AMPH_NO_FAILURE in device mode), the malformed token's byte offset
 *   INSIDE OBJECT o's OWN TEXT, or text_lens[o] when the text is well-formed
 *   but does not hold P_o pairs.  Whitespace between tokens and "b","a" member
 *   order are accepted as there; magnitudes must be < 2^128.  An object with a
 *   reported fault has unspecified contents in ITS OWN rows of mag16 / neg;
 *   every other object's rows and verdict are written as if it were alone.
 *   What lies in the rest of a slot or in a gap is never read.  A faulty or
 *   whitespace-bearing text may cost its neighbours time, never a byte.
 *
 *   Host mode: the tables are checked first; a breach returns AMPH_E_PARAM
 *   with nothing launched.  ONE page-locked image goes to the device and one
 *   comes back; a call that fits the small-call arena is built there and moves
 *   nothing (amph_exchange_batch_copies counts).  Decode status: AMPH_E_PARAM
 *   if any text was refused, AMPH_E_LEN if the only failures are count
 *   mismatches; amph_last_error names the first such object, its offset and
 *   how many were refused.  The diffs of every clean object are written either
 *   way.
 *
 *   AMPH_F_DEVICE: the tables, out_lens, text_lens and bad_index are 8-byte
 *   aligned device arrays, mag16, out and texts 16-byte aligned (AMPH_E_PARAM
 *   otherwise); asynchronous on `stream`, with the single calls' scratch and
 *   ordering.  bad_index is reset to AMPH_NO_FAILURE unless AMPH_F_ACCUMULATE is
 *   set (then the verdicts are min-combined into it).  Launch sizes come from
 *   npairs_total, n_objects and texts_len alone.  The tables' contract is the
 *   CALLER's: whatever they hold, nothing outside mag16's 32 npairs_total
 *   bytes, neg's 2 npairs_total bytes and the 16-byte units of texts that hold
 *   a byte of [0, texts_len) is read, and nothing outside out[0, out_cap),
 *   those diff arrays and entries [0, n_objects) of out_lens / bad_index is
 *   written.
 *
 *   AMPH_F_HOST_IO is refused; AMPH_F_ACCUMULATE is accepted by the device
 *   decode only.  A multi-device context runs these calls on devices[0].
 *   n_objects == 0 returns AMPH_OK and launches nothing.  The number of kernel
 *   launches of a call does not depend on n_objects. */
int amph_exchange_encode_packed(amph_ctx* ctx, const uint8_t* mag16, const uint8_t* neg, size_t npairs_total,
                                const uint64_t* pair_offsets, const uint64_t* text_offsets, size_t n_objects,
                                char* out, size_t out_cap, uint64_t* out_lens, uint32_t flags, void* stream);

int amph_exchange_decode_packed(amph_ctx* ctx, const char* texts, size_t texts_len, const uint64_t* pair_offsets,
                                const uint64_t* text_offsets, const uint64_t* text_lens, size_t n_objects,
                                size_t npairs_total, uint8_t* mag16, uint8_t* neg, int64_t* bad_index,
                                uint32_t flags, void* stream);

/* ---- GATHER form, host memory only (any flag: AMPH_E_PARAM) ---------------------
 * Encode: mag16[o] / neg[o] = object o's npairs[o] pairs, out[o] a buffer of
 * out_caps[o] characters.  Every out_lens[o] is set to the text's length.  An
 * out_caps[o] below it returns AMPH_E_LEN naming the first such object: the
 * texts that fit are written, the others' buffers untouched.
 * Decode: texts[o] of lens[o] characters, expected to hold npairs[o] pairs,
 * into mag16[o] / neg[o]; bad_index and the status as the packed form's.
 * The library gathers into its page-locked image (dense slots), runs the
 * packed path once and scatters the results. */
int amph_exchange_encode_batch(amph_ctx* ctx, const uint8_t* const* mag16, const uint8_t* const* neg,
                               const size_t* npairs, size_t n_objects, char* const* out, const size_t* out_caps,
                               uint64_t* out_lens, uint32_t flags);

int amph_exchange_decode_batch(amph_ctx* ctx, const char* const* texts, const size_t* lens, const size_t* npairs,
                               size_t n_objects, uint8_t* const* mag16, uint8_t* const* neg, int64_t* bad_index,
                               uint32_t flags);

/* Host-device copies (hipMemcpy calls) the host mode of the four calls above
 * has issued on this context so far: 2 per staged call, whatever n_objects is,
 * and 0 for a call that fits the small-call arena. */
uint64_t amph_exchange_batch_copies(const amph_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* AMPHORA_EXCHANGE_BATCH_H_ */
