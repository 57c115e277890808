"""Host-side mirror of the client arithmetic (amphora-java-client), routed to
the HIP kernels through the C ABI.

Mirrors:
* SecretShareUtil            amphora-java-client/.../client/SecretShareUtil.java:33-157
  (of :48-51, maskInput :65-68, recombineObject :70-90, verifySecrets :102-141)
* DefaultAmphoraClient.verifyOutputDeliveryObjects :476-505 and the
  arithmetic of createSecret :150-160 / getSecret :206-217.

Java BigIntegers are Python ints here.  Host-side obligations of the
boundary: arbitrary ints are reduced mod p before packing into
16-byte words; canonical outputs are unpacked back to ints.  No field
arithmetic happens in Python.
"""
from __future__ import annotations

from typing import List, Sequence

import numpy as np

from . import _lib
from .entities import (AmphoraClientException, IntegrityVerificationException, MaskedInput,
                       MaskedInputData, MaskedInputWords, OutputDeliveryObject, Secret, WORD_WIDTH)

_MASK128 = (1 << 128) - 1


def pack(values: Sequence[int], prime: int = None) -> np.ndarray:
    """ints -> (W, 16) LE words; reduced mod prime when given (BigInteger.mod)."""
    if prime is not None:
        values = [v % prime if (v < 0 or v > _MASK128) else v for v in values]
    buf = b"".join(int(v).to_bytes(16, "little") for v in values)
    return np.frombuffer(buf, np.uint8).reshape(-1, 16).copy() if buf else np.zeros((0, 16), np.uint8)


def unpack(words) -> List[int]:
    if hasattr(words, "is_cuda"):
        words = words.cpu().numpy()
    b = np.ascontiguousarray(words, np.uint8).tobytes()
    return [int.from_bytes(b[i:i + 16], "little") for i in range(0, len(b), 16)]


class SecretShareUtil:
    """Client SecretShareUtil; ``of`` keeps the reference factory signature."""

    def __init__(self, ctx: _lib.Context):
        self._ctx = ctx

    @classmethod
    def of(cls, prime: int, r: int, r_inv: int, device: int = 0) -> "SecretShareUtil":
        if prime is None or r is None or r_inv is None:
            raise TypeError("prime, r and rInv must not be null")  # @NonNull :48-49
        return cls(_lib.Context(prime, r, r_inv, device))

    @property
    def prime(self) -> int:
        return self._ctx.prime

    @property
    def r(self) -> int:
        return self._ctx.r

    @property
    def r_inv(self) -> int:
        return self._ctx.r_inv

    @property
    def context(self) -> _lib.Context:
        return self._ctx

    def mask_input(self, secret: int, input_mask: int) -> MaskedInputData:
        """maskInput :65-68: MaskedInputData.of(toGfp((secret - inputMask) mod p))."""
        return self.mask_inputs([secret], [input_mask])[0]

    def mask_inputs(self, secrets: Sequence[int], input_masks: Sequence[int]) -> List[MaskedInputData]:
        out = self._ctx.mask_words(pack(secrets, self.prime), pack(input_masks, self.prime))
        return [MaskedInputData.of(bytes(w)) for w in out]

    def recombine_object(self, shares: Sequence[bytes]) -> List[int]:
        """recombineObject :70-90 (word count from shares[0], trailing bytes ignored)."""
        if len(shares) == 0:
            return []
        W = len(shares[0]) // WORD_WIDTH
        views = [_lib.words_view(s)[:W] for s in shares]
        if any(v.shape[0] < W for v in views):
            raise IndexError("share arrays shorter than the first")
        return unpack(self._ctx.recombine(views))

    def verify_secrets(self, secrets, rs, us, vs, ws) -> None:
        """verifySecrets :102-141 (argument order of the Java method)."""
        n = len(secrets)
        p = self.prime
        # host precheck: a w/u outside [0, p) can never equal a reduced product
        pre = [i for i in range(n) if not (0 <= ws[i] < p and 0 <= us[i] < p)]
        ok_w = [w if 0 <= w < p else 0 for w in ws]
        ok_u = [u if 0 <= u < p else 0 for u in us]
        ff = self._ctx.verify(pack(secrets, p), pack(rs, p), pack(ok_u), pack(vs, p), pack(ok_w))
        cand = [i for i in ([ff] if ff >= 0 else []) + pre[:1]]
        if cand:
            i = min(cand)
            raise IntegrityVerificationException(
                self.failure_message(secrets[i], rs[i], us[i], vs[i], ws[i]))

    def failure_message(self, y, r, u, v, w) -> str:
        """Message of SecretShareUtil.java:116-129; products computed natively."""
        p = self.prime
        fits = all(0 <= x <= _MASK128 for x in (y, r, u, v, w))
        if fits:
            return self._ctx.verify_message(y, r, u, v, w)
        msg = self._ctx.verify_message(y % p, r % p, u % p, v % p, w % p)
        tail = msg.split("\n")[-1]  # "\t{w} = {aw}   &&   {u} = {au}"
        aw = tail.split("   &&   ")[0].split(" = ")[1]
        au = tail.split("   &&   ")[1].split(" = ")[1]
        return ("Verification of secret has failed:\n\t%d = %d * %d   &&   %d = %d * %d\n"
                "\t%d = %s   &&   %d = %s" % (w, y, r, u, v, r, w, aw, u, au))


def _odo_arrays(odos: Sequence[OutputDeliveryObject]):
    """Every party's five fields as they are, with their own byte lengths:
    the C ABI applies recombineObject's copyOfRange rules to ragged parties
    (client SecretShareUtil.java:75,87-88), so nothing is cut here."""
    return [tuple(o.fields()) for o in odos]


def _words(arrays) -> int:
    return _lib.byte_len(arrays[0][0]) // WORD_WIDTH  # party 0's word count (:75)


def verify_output_delivery_objects(util: SecretShareUtil,
                                   odos: Sequence[OutputDeliveryObject]) -> List[int]:
    """DefaultAmphoraClient.verifyOutputDeliveryObjects :476-505, fused into one
    kernel (K_RV): 5 recombines + verify, returns the canonical secrets."""
    arrays = _odo_arrays(odos)
    y, ff = _native(util.context.recombine_verify, arrays)
    if ff >= 0:
        _raise_for(util, arrays, ff)
    return unpack(y)


def _native(fn, *args):
    """A C-ABI call whose AMPH_E_RANGE (a party's word starting past the end
    of its array) is Java's ArrayIndexOutOfBoundsException (IndexError)."""
    try:
        return fn(*args)
    except _lib.AmphoraNativeError as e:
        if e.status == _lib.AMPH_E_RANGE:
            raise IndexError(str(e)) from e
        raise


def _raise_for(util: SecretShareUtil, arrays, i: int):
    """Re-render the reference message for word i from its recombined values:
    each party's word i is Arrays.copyOfRange(field, 16 i, 16 i + 16) --
    zero-padded when the party's array ends inside it -- exactly what
    recombineObject hands fromGfp (amph_recombine_object on those slices)."""
    lo, hi = WORD_WIDTH * i, WORD_WIDTH * (i + 1)
    vals = [unpack(util.context.recombine_object([_slice(a[k], lo, hi) for a in arrays]))[0]
            for k in range(5)]
    y, r, v, w, u = vals
    raise IntegrityVerificationException(util.failure_message(y, r, u, v, w))


def _slice(x, lo: int, hi: int):
    if hasattr(x, "is_cuda"):
        return x.reshape(-1)[lo:hi]
    return bytes(memoryview(x).cast("B")[lo:hi]) if not isinstance(x, bytes) else x[lo:hi]


def create_masked_input(util: SecretShareUtil, secret: Secret,
                        mask_odos: Sequence[OutputDeliveryObject]) -> MaskedInput:
    """Arithmetic of DefaultAmphoraClient.createSecret :150-160 fused into one
    kernel (K_MASK): verify the Input Mask ODOs, then maskInput per word.
    More secret words than masks: the C ABI verifies every mask first
    (:153) and only then reports the length (AMPH_E_LEN), which is the
    reference's IndexOutOfBoundsException from inputMasks.get(i) (:155-157)."""
    arrays = _odo_arrays(mask_odos)
    W = _words(arrays)
    try:
        masked, ff = _native(util.context.mask_input, arrays, pack(secret.data, util.prime))
    except _lib.AmphoraNativeError as e:
        if e.status == _lib.AMPH_E_LEN and secret.size() > W:
            raise IndexError("Index %d out of bounds for length %d" % (W, W)) from e
        raise
    if ff >= 0:
        _raise_for(util, arrays, ff)
    return MaskedInput(secret.secret_id, MaskedInputWords(masked), list(secret.tags))


# ---- many secrets per launch ------------------------------------------------------
# The reference client has no multi-secret method: K getSecret / createSecret
# calls each return their own secret or throw their own exception.  The batch
# functions keep that contract -- one entry per secret, the value or the
# exception the single function would raise -- over ONE launch
# (amph_recombine_verify_batch / amph_mask_input_batch).

def _outcome(fn, *args):
    try:
        return fn(*args)
    except Exception as e:  # the caller gets it as this secret's entry
        return e


def _regular(arrays, n_parties: int) -> bool:
    """All 5 n fields of one byte length: what the gathered ABI calls take.
    Anything else (ragged parties, another party count) keeps the single
    call's semantics and exceptions by going through the single call."""
    if len(arrays) != n_parties or n_parties == 0:
        return False
    b0 = _lib.byte_len(arrays[0][0])
    return all(len(a) == 5 and all(_lib.byte_len(f) == b0 for f in a) for a in arrays)


def _batch_outcomes(util, arrays_list, regular, run, finish, single):
    out = [None] * len(arrays_list)
    idx = [o for o, r in enumerate(regular) if r]
    if idx:
        words, ff = run(idx)
        for k, o in enumerate(idx):
            if ff[k] >= 0:
                out[o] = _outcome(_raise_for, util, arrays_list[o], int(ff[k]))
            else:
                out[o] = finish(o, words[k])
    for o, r in enumerate(regular):
        if not r:
            out[o] = _outcome(single, o)
    return out


def verify_output_delivery_objects_batch(util: SecretShareUtil,
                                         list_of_odo_lists: Sequence[Sequence[OutputDeliveryObject]]):
    """verify_output_delivery_objects for K secrets in one launch.  Returns a
    list with one entry per secret: the canonical secrets (List[int]), or the
    exception the single function would raise for that secret (for a MAC
    failure, IntegrityVerificationException with the reference's message)."""
    arrays_list = [_odo_arrays(odos) for odos in list_of_odo_lists]
    n = next((len(a) for a in arrays_list if len(a)), 0)
    regular = [_regular(a, n) for a in arrays_list]
    return _batch_outcomes(
        util, arrays_list, regular,
        lambda idx: util.context.recombine_verify_batch([arrays_list[o] for o in idx]),
        lambda o, y: unpack(y),
        lambda o: verify_output_delivery_objects(util, list_of_odo_lists[o]))


def create_masked_inputs(util: SecretShareUtil, secrets: Sequence[Secret],
                         list_of_mask_odo_lists: Sequence[Sequence[OutputDeliveryObject]]):
    """create_masked_input for K secrets in one launch: one entry per secret,
    the MaskedInput or the exception create_masked_input would raise.  A
    secret whose word count differs from its mask count goes through the
    single call (which verifies the masks before it reports the length)."""
    if len(secrets) != len(list_of_mask_odo_lists):
        raise ValueError("one list of Input Mask ODOs per secret")
    arrays_list = [_odo_arrays(odos) for odos in list_of_mask_odo_lists]
    n = next((len(a) for a in arrays_list if len(a)), 0)
    regular = [_regular(a, n) and secrets[o].size() == _words(a) for o, a in enumerate(arrays_list)]
    return _batch_outcomes(
        util, arrays_list, regular,
        lambda idx: util.context.mask_input_batch([arrays_list[o] for o in idx],
                                                  [pack(secrets[o].data, util.prime) for o in idx]),
        lambda o, m: MaskedInput(secrets[o].secret_id, MaskedInputWords(m), list(secrets[o].tags)),
        lambda o: create_masked_input(util, secrets[o], list_of_mask_odo_lists[o]))


def _texts_and_words(bodies):
    """Field texts of every party's body and the word count.  A malformed
    body -- a field that is not a whole number of 16-byte words, or fields of
    unequal length within or across parties -- is an AmphoraClientException,
    as Jackson's deserialisation failure is in the reference
    (DefaultAmphoraClient.java:206-217 via AmphoraCommunicationClient)."""
    from . import wire
    texts = [wire.odo_field_texts(b)[0] for b in bodies]
    try:
        W = wire.words_of_b64(len(texts[0][0]), texts[0][0][-2:])
    except ValueError as e:
        raise AmphoraClientException(str(e)) from e
    n0 = len(texts[0][0])
    if any(len(f) != n0 for t in texts for f in t):
        # OutputDeliveryObject's constructor (OutputDeliveryObject.java:55-96)
        raise AmphoraClientException("The provided shares must be of the same length")
    return texts, W


def _wire_call(fn, *args, **kw):
    """A fused wire-kernel call; a bad character or a length mismatch in some
    party's text becomes AmphoraClientException."""
    try:
        return fn(*args, **kw)
    except ValueError as e:  # an illegal base64 character in some party's body
        raise AmphoraClientException(str(e)) from e
    except _lib.AmphoraNativeError as e:
        if e.status == _lib.AMPH_E_LEN:
            raise AmphoraClientException(str(e)) from e
        raise


def _raise_for_texts(util: SecretShareUtil, texts, i: int):
    # failure path only: decode the fields and render the reference message
    arrays = [tuple(util.context.base64_decode(t) for t in ts) for ts in texts]
    _raise_for(util, arrays, i)


def verify_vss_json(util: SecretShareUtil, bodies: Sequence[str], secret_id=None):
    """getSecret from the parties' VerifiableSecretShare JSON bodies
    (DefaultAmphoraClient.java:206-217 incl. Jackson's base64 decode of each
    field): the base64 member strings go to the fused K_RV wire kernel
    (amph_recombine_verify_b64) as they are.  Returns (secretId, tags,
    canonical secrets).  As in the reference (:213-216) the secretId is the
    one requested (`secret_id`; party 0's body only when none is given) and
    only the tags come from party 0's body."""
    from . import wire
    texts, W = _texts_and_words(bodies)
    y, ff, _ = _wire_call(util.context.recombine_verify_b64, texts, W)
    if ff >= 0:
        _raise_for_texts(util, texts, ff)
    sid, tags = wire.vss_metadata(bodies[0], wire.odo_field_texts(bodies[0])[1])
    return (sid if secret_id is None else secret_id), tags, unpack(y)


def create_masked_input_json(util: SecretShareUtil, secret: Secret, odo_bodies: Sequence[str]) -> str:
    """createSecret from the parties' OutputDeliveryObject JSON bodies
    (GET /input-masks) to the MaskedInput JSON body (POST /masked-inputs):
    verify the masks + maskInput + the per-word base64 records in one fused
    launch (amph_mask_input_b64)."""
    from . import wire
    texts, W = _texts_and_words(odo_bodies)
    try:
        # more secret words than masks: the ABI decodes and verifies every
        # mask first (a MAC failure comes back as ff), and only then reports
        # the length -- the reference's order (:153 before :155-157)
        _, rec, ff, _ = _wire_call(util.context.mask_input_b64, texts, W, pack(secret.data, util.prime),
                                   records=True)
    except AmphoraClientException as e:
        if secret.size() > W and isinstance(e.__cause__, _lib.AmphoraNativeError) \
                and e.__cause__.status == _lib.AMPH_E_LEN:
            raise IndexError("Index %d out of bounds for length %d" % (W, W)) from e.__cause__
        raise
    if ff >= 0:
        _raise_for_texts(util, texts, ff)
    return wire.records_to_masked_input_json(secret.secret_id, rec, secret.tags)


# ---- many secrets per launch, from their JSON bodies --------------------------------
# verify_vss_json / create_masked_input_json for K secrets over ONE launch
# (amph_recombine_verify_b64_batch / amph_mask_input_b64_batch): one entry per
# secret, the value or the exception the single function raises for it.

def _body_texts(bodies):
    """(texts, W) of one secret's bodies, or the exception _texts_and_words
    raises (that secret then goes through the single function, which raises
    it again as its own)."""
    try:
        return _texts_and_words(bodies)
    except Exception:  # malformed JSON, unequal field lengths, not whole words
        return None, None


def _wire_batch_outcomes(util, parsed, regular, run, finish, single):
    out = [None] * len(parsed)
    idx = [o for o, r in enumerate(regular) if r]
    if idx:
        values, ff, bad = run(idx)
        for k, o in enumerate(idx):
            texts, W = parsed[o]
            if bad[k] >= 0:
                out[o] = AmphoraClientException(_lib.wire_bad_char_message(int(bad[k]), W))
            elif ff[k] >= 0:
                out[o] = _outcome(_raise_for_texts, util, texts, int(ff[k]))
            else:
                out[o] = _outcome(finish, o, values[k])
    for o, r in enumerate(regular):
        if not r:
            out[o] = _outcome(single, o)
    return out


def verify_vss_json_batch(util: SecretShareUtil, list_of_bodies_lists, secret_ids=None):
    """verify_vss_json for K secrets in one launch.  Returns one entry per
    secret: (secretId, tags, canonical secrets), or the exception
    verify_vss_json raises for that secret -- IntegrityVerificationException
    with the reference's message for a MAC failure, AmphoraClientException with
    the single call's text for an illegal base64 character.  A secret with
    another party count than the first, or with malformed bodies, goes
    through verify_vss_json itself."""
    from . import wire
    parsed = [_body_texts(b) for b in list_of_bodies_lists]
    n = next((len(t) for t, _ in parsed if t), 0)
    regular = [t is not None and len(t) == n for t, _ in parsed]
    sid_of = lambda o: None if secret_ids is None else secret_ids[o]  # noqa: E731

    def finish(o, y):
        b0 = list_of_bodies_lists[o][0]
        sid, tags = wire.vss_metadata(b0, wire.odo_field_texts(b0)[1])
        return (sid if sid_of(o) is None else sid_of(o)), tags, unpack(y)

    return _wire_batch_outcomes(
        util, parsed, regular,
        lambda idx: util.context.recombine_verify_b64_batch([parsed[o][0] for o in idx], [parsed[o][1] for o in idx]),
        finish,
        lambda o: verify_vss_json(util, list_of_bodies_lists[o], sid_of(o)))


def create_masked_inputs_from_bodies(util: SecretShareUtil, secrets: Sequence[Secret], list_of_odo_bodies_lists):
    """create_masked_input_json for K secrets in one launch: one entry per
    secret, the MaskedInput JSON body or the exception create_masked_input_json
    raises for that secret.  A secret whose word count differs from its mask
    count goes through the single function (which verifies the masks before
    it reports the length), as do other party counts and malformed bodies."""
    from . import wire
    if len(secrets) != len(list_of_odo_bodies_lists):
        raise ValueError("one list of Input Mask ODO bodies per secret")
    parsed = [_body_texts(b) for b in list_of_odo_bodies_lists]
    n = next((len(t) for t, _ in parsed if t), 0)
    regular = [t is not None and len(t) == n and secrets[o].size() == W for o, (t, W) in enumerate(parsed)]

    def run(idx):
        _, rec, ff, bad = util.context.mask_input_b64_batch(
            [parsed[o][0] for o in idx], [parsed[o][1] for o in idx],
            [pack(secrets[o].data, util.prime) for o in idx], records=True)
        return rec, ff, bad

    return _wire_batch_outcomes(
        util, parsed, regular, run,
        lambda o, rec: wire.records_to_masked_input_json(secrets[o].secret_id, rec, secrets[o].tags),
        lambda o: create_masked_input_json(util, secrets[o], list_of_odo_bodies_lists[o]))


def create_masked_input_body(util: SecretShareUtil, secret: Secret, odo_bodies: Sequence[str]) -> str:
    """create_masked_input_json with the "data" array text written by the
    kernel itself (amph_mask_input_json): the records leave the GPU already
    framed as [{"value":"..."},...], so no host pass frames them.  Same body,
    same exceptions."""
    import json
    from . import wire
    texts, W = _texts_and_words(odo_bodies)
    try:
        data, ff, _ = _wire_call(util.context.mask_input_json, texts, W, pack(secret.data, util.prime))
    except AmphoraClientException as e:
        if secret.size() > W and isinstance(e.__cause__, _lib.AmphoraNativeError) \
                and e.__cause__.status == _lib.AMPH_E_LEN:
            raise IndexError("Index %d out of bounds for length %d" % (W, W)) from e.__cause__
        raise
    if ff >= 0:
        _raise_for_texts(util, texts, ff)
    tj = json.dumps([wire._tag_obj(t) for t in secret.tags], separators=(",", ":"))
    return '{"secretId":"%s","data":%s,"tags":%s}' % (secret.secret_id, data.decode("ascii"), tj)


def create_masked_input_bodies(util: SecretShareUtil, secrets: Sequence[Secret], list_of_odo_bodies_lists):
    """create_masked_input_body for K secrets in one launch
    (amph_mask_input_json_batch): every "data" array text leaves the GPU
    framed, no host pass frames K bodies.  One entry per secret, equal to
    what create_masked_inputs_from_bodies returns for it: the MaskedInput JSON
    body or the exception the single function raises."""
    import json
    from . import wire
    if len(secrets) != len(list_of_odo_bodies_lists):
        raise ValueError("one list of Input Mask ODO bodies per secret")
    parsed = [_body_texts(b) for b in list_of_odo_bodies_lists]
    n = next((len(t) for t, _ in parsed if t), 0)
    regular = [t is not None and len(t) == n and secrets[o].size() == W for o, (t, W) in enumerate(parsed)]

    def run(idx):
        return util.context.mask_input_json_batch(
            [parsed[o][0] for o in idx], [parsed[o][1] for o in idx],
            [pack(secrets[o].data, util.prime) for o in idx])

    def finish(o, data):
        tj = json.dumps([wire._tag_obj(t) for t in secrets[o].tags], separators=(",", ":"))
        return '{"secretId":"%s","data":%s,"tags":%s}' % (secrets[o].secret_id, data.decode("ascii"), tj)

    return _wire_batch_outcomes(
        util, parsed, regular, run, finish,
        lambda o: create_masked_input_body(util, secrets[o], list_of_odo_bodies_lists[o]))


class ResponseSession:
    """The parties' response bodies consumed as they arrive
    (include/amphora_client_session.h): every body's five base64 member
    strings go into the running sums on the GPU at once (add_body, one launch
    per party; any thread may hand in its own party), and secret /
    masked_input_json / masked_input_body finish from the sums -- the values,
    bodies and exceptions of verify_vss_json / create_masked_input_json /
    create_masked_input_body on the same bodies.  The first body fixes the
    word count; only party 0's body is kept as text (its tags)."""

    def __init__(self, util: SecretShareUtil, n_parties: int):
        import threading
        self._util, self._n = util, n_parties
        self._lock = threading.Lock()
        self._session = None
        self._words = None
        self._body0 = None
        self._error = None  # the first malformed body / bad character, raised by the finish

    @property
    def words(self):
        return self._words

    def add_body(self, party_index: int, body) -> None:
        from . import wire
        texts = wire.odo_field_texts(body)[0]
        if party_index == 0:
            self._body0 = body
        with self._lock:
            try:
                if self._session is None:
                    try:
                        W = wire.words_of_b64(len(texts[0]), texts[0][-2:])
                    except ValueError as e:
                        raise AmphoraClientException(str(e)) from e
                    self._session = self._util.context.client_begin(W, self._n)
                    self._words = W
                if any(len(f) != len(texts[0]) for f in texts):
                    raise AmphoraClientException("The provided shares must be of the same length")
            except AmphoraClientException as e:
                self._error = self._error or e
                raise
            session = self._session
        try:
            _wire_call(session.party, party_index, texts)
        except AmphoraClientException as e:
            if isinstance(e.__cause__, _lib.AmphoraNativeError):  # another length than the first body's
                e = AmphoraClientException("The provided shares must be of the same length")
                with self._lock:
                    self._error = self._error or e
                raise e from None
            raise  # a bad character: the session keeps the smallest, the finish reports it

    def _finish(self, name: str, *args, **kw):
        if self._error is not None:
            raise self._error
        if self._session is None:
            raise AmphoraClientException("no response body was added")
        return _wire_call(getattr(self._session, name), *args, **kw)

    def _raise_for(self, i: int):
        y, r, v, w, u = self._session.word(i)
        raise IntegrityVerificationException(self._util.failure_message(y, r, u, v, w))

    def secret(self, secret_id=None):
        """-> (secretId, tags, canonical secrets), as verify_vss_json."""
        from . import wire
        y, ff, _ = self._finish("finish_verify")
        if ff >= 0:
            self._raise_for(ff)
        sid, tags = wire.vss_metadata(self._body0, wire.odo_field_texts(self._body0)[1])
        return (sid if secret_id is None else secret_id), tags, unpack(y)

    def _mask(self, secret: Secret, fn_name: str, **kw):
        W = self._words
        try:
            res = self._finish(fn_name, pack(secret.data, self._util.prime), **kw)
        except AmphoraClientException as e:
            if W is not None and secret.size() > W and isinstance(e.__cause__, _lib.AmphoraNativeError) \
                    and e.__cause__.status == _lib.AMPH_E_LEN:
                raise IndexError("Index %d out of bounds for length %d" % (W, W)) from e.__cause__
            raise
        if res[-2] >= 0:
            self._raise_for(res[-2])
        return res

    def masked_input_json(self, secret: Secret) -> str:
        """-> the MaskedInput JSON body, as create_masked_input_json."""
        from . import wire
        _, rec, _, _ = self._mask(secret, "finish_mask", records=True)
        return wire.records_to_masked_input_json(secret.secret_id, rec, secret.tags)

    def masked_input_body(self, secret: Secret) -> str:
        """-> the MaskedInput JSON body, as create_masked_input_body."""
        import json
        from . import wire
        data, _, _ = self._mask(secret, "finish_mask_json")
        tj = json.dumps([wire._tag_obj(t) for t in secret.tags], separators=(",", ":"))
        return '{"secretId":"%s","data":%s,"tags":%s}' % (secret.secret_id, data.decode("ascii"), tj)

    def close(self):
        if self._session is not None:
            self._session.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class ResponseSessions:
    """ResponseSession for K secrets (include/amphora_client_batch.h): every
    party hands in its K response bodies at once (add_bodies: the bodies go to
    the session as they are -- include/amphora_client_bodies.h: each is scanned
    in C for its five base64 members and the kernel decodes them where they
    lie, ONE launch; any thread may hand in its own party), and
    secrets / masked_input_bodies finish from the sums -- one entry per
    secret, the value or that secret's exception, as verify_vss_json_batch /
    create_masked_input_bodies return on the same bodies.  The first party's K
    bodies fix the word table; only party 0's bodies are kept as text (their
    tags).

    in_place=False, or any body of a call that the scanner refuses (an escape
    in a member, a duplicate, a null ...) or whose members are not ASCII:
    that call's 5 K member strings are cut out by wire.odo_field_texts and
    gathered into five slotted buffers, the path that defines every outcome."""

    def __init__(self, util: SecretShareUtil, n_parties: int, in_place: bool = True):
        import threading
        self._util, self._n, self._in_place = util, n_parties, in_place
        self._lock = threading.Lock()
        self._session = None
        self._words = None   # per object, fixed by the first party that arrives
        self._bodies0 = None
        self._errors = None  # per object: the first malformed body's exception

    @property
    def words(self):
        return self._words

    def _begin(self, shapes):
        """shapes: per object (characters of its secretShares, its last two)."""
        from . import wire
        words, errors = [], []
        for nchars, last2 in shapes:
            try:
                words.append(wire.words_of_b64(nchars, last2))
                errors.append(None)
            except ValueError as e:  # not whole words: this secret alone fails
                words.append(0)
                errors.append(AmphoraClientException(str(e)))
        self._words, self._errors = words, errors
        self._session = self._util.context.clients_begin(np.concatenate([[0], np.cumsum(words)]).astype(np.uint64),
                                                         self._n)

    def add_bodies(self, party_index: int, bodies) -> None:
        """Party `party_index`'s K bodies (one per secret, in the order of the
        first party's).  A malformed body or a bad character fails its own
        secret only; the finish reports it."""
        from . import wire
        scans = self._scan(bodies) if self._in_place else None
        if scans is not None:
            return self._add_in_place(party_index, bodies, *scans)
        bodies = [b if isinstance(b, str) else bytes(b).decode("utf-8") for b in bodies]
        texts = [wire.odo_field_texts(b)[0] for b in bodies]
        if party_index == 0:
            self._bodies0 = list(bodies)
        with self._lock:
            if self._session is None:
                self._begin([(len(t[0]), t[0][-2:]) for t in texts])
            if len(texts) != len(self._words):
                raise AmphoraClientException("party %d answered %d of %d secrets" % (
                    party_index, len(texts), len(self._words)))
            s = self._session
            bufs = np.zeros((5, max(s.field_chars, 1)), np.uint8)
            for o, (t, nc) in enumerate(zip(texts, s.field_lens())):
                if self._errors[o] is not None:
                    continue
                if any(len(f) != nc for f in t):  # its slot stays 0: an illegal character in this object alone
                    self._errors[o] = AmphoraClientException("The provided shares must be of the same length")
                    continue
                at = int(s.field_offsets[o])
                for k in range(5):
                    f = t[k].encode("ascii", errors="replace") if isinstance(t[k], str) else bytes(t[k])
                    bufs[k, at:at + nc] = np.frombuffer(f, np.uint8)
        s.party(party_index, [bufs[k, :s.field_chars] for k in range(5)], status=True)

    @staticmethod
    def _scan(bodies):
        """-> (the bodies as bytes, starts (K, 5), lens (K, 5)), or None when
        any body is not plain or a member holds a non-ASCII byte (the gather
        path replaces such a character, one for one: its verdict is the
        reference)."""
        raw = [b.encode("utf-8") if isinstance(b, str) else bytes(b) for b in bodies]
        starts, lens = np.empty((len(raw), 5), np.uint64), np.empty((len(raw), 5), np.uint64)
        try:
            for o, r in enumerate(raw):
                starts[o], lens[o] = _lib.bodies_scan(r)
        except _lib.BodyNotPlain:
            return None
        for o, (b, r) in enumerate(zip(bodies, raw)):
            if not (b.isascii() if isinstance(b, str) else r.isascii()):  # (str.isascii costs nothing)
                if not all(r[int(a):int(a) + int(n)].isascii() for a, n in zip(starts[o], lens[o])):
                    return None
        return raw, starts, lens

    def _add_in_place(self, party_index: int, bodies, raw, starts, lens) -> None:
        if party_index == 0:
            self._bodies0 = [b if isinstance(b, str) else r.decode("utf-8") for b, r in zip(bodies, raw)]
        with self._lock:
            if self._session is None:
                self._begin([(int(n[0]), r[int(a[0]) + max(int(n[0]) - 2, 0):int(a[0]) + int(n[0])].decode("ascii"))
                             for r, a, n in zip(raw, starts, lens)])
            if len(raw) != len(self._words):
                raise AmphoraClientException("party %d answered %d of %d secrets" % (
                    party_index, len(raw), len(self._words)))
            s = self._session
            for o, nc in enumerate(s.field_lens()):
                if self._errors[o] is None and (lens[o] != nc).any():
                    self._errors[o] = AmphoraClientException("The provided shares must be of the same length")
                if self._errors[o] is not None:  # absent: what a slot left zero reports, in this object alone
                    starts[o] = _lib.AMPH_BODY_ABSENT
        s.party_bodies(party_index, raw, starts, status=True)

    def _outcomes(self, ff, bad, value):
        out = []
        for o, W in enumerate(self._words):
            if self._errors[o] is not None:
                out.append(self._errors[o])
            elif bad[o] >= 0:
                out.append(AmphoraClientException(_lib.wire_bad_char_message(int(bad[o]), W)))
            elif ff[o] >= 0:
                y, r, v, w, u = self._session.word(o, int(ff[o]))
                out.append(IntegrityVerificationException(self._util.failure_message(y, r, u, v, w)))
            else:
                out.append(_outcome(value, o))
        return out

    def _need_session(self):
        if self._session is None:
            raise AmphoraClientException("no response body was added")
        return self._session

    def secrets(self, secret_ids=None):
        """-> one entry per secret: (secretId, tags, canonical secrets) or the
        exception verify_vss_json raises for it."""
        from . import wire
        s = self._need_session()
        y, ff, bad = s.finish_verify()
        wo = s.word_offsets

        def value(o):
            b0 = self._bodies0[o]
            sid, tags = wire.vss_metadata(b0, wire.odo_field_texts(b0)[1])
            return (sid if secret_ids is None else secret_ids[o]), tags, unpack(y[int(wo[o]):int(wo[o + 1])])

        return self._outcomes(ff, bad, value)

    def masked_input_bodies(self, secrets: Sequence[Secret]):
        """-> one entry per secret: the MaskedInput JSON body or the exception
        create_masked_input_body raises for it.  A secret with fewer words
        than its masks is padded for the launch (every mask is verified) and
        its text cut after its own last record; one with more is an
        IndexError once its masks have verified, as in the single call."""
        import json
        from . import wire
        s = self._need_session()
        if len(secrets) != len(self._words):
            raise ValueError("one secret per object of the session")
        padded = np.zeros((s.words, 16), np.uint8)
        for o, sec in enumerate(secrets):
            W, a = self._words[o], int(s.word_offsets[o])
            m = min(W, sec.size())
            if m:
                padded[a:a + m] = pack(sec.data[:m], self._util.prime)
        text, ff, bad = s.finish_mask_json(padded)
        framed = s.split_upload(text)

        def value(o):
            sec, W = secrets[o], self._words[o]
            if sec.size() > W:
                raise IndexError("Index %d out of bounds for length %d" % (W, W))
            S = sec.size()
            data = framed[o] if S == W else (framed[o][:37 * S] + b"]" if S else b"[]")
            tj = json.dumps([wire._tag_obj(t) for t in sec.tags], separators=(",", ":"))
            return '{"secretId":"%s","data":%s,"tags":%s}' % (sec.secret_id, data.decode("ascii"), tj)

        return self._outcomes(ff, bad, value)

    def close(self):
        if self._session is not None:
            self._session.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def get_secret_data(util: SecretShareUtil, odos: Sequence[OutputDeliveryObject]) -> List[int]:
    """getSecret :206-217 arithmetic (alias of verify_output_delivery_objects)."""
    return verify_output_delivery_objects(util, odos)
