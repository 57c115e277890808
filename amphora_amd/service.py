"""Host-side mirror of the party (amphora-service) arithmetic, routed to the
HIP kernels through the C ABI.

Mirrors:
* calculation/SecretShareUtil.convertToSecretShare
      amphora-service/.../calculation/SecretShareUtil.java:30-107     (K_CONV)
* calculation/OutputDeliveryService.computeOutputDeliveryObject
      amphora-service/.../calculation/OutputDeliveryService.java:57-286
      local parts: K_ODO_PRE -> exchange -> open (recombineDiffs) + K_ODO_POST,
      the last two fused in one launch (amph_open_post)
* persistence/cache/InputMaskCachingService.getInputMasksAsOutputDeliveryObject
      InputMaskCachingService.java:77-99 (value halves of the mask tuples)

Castor, Redis and the inter-VCP HTTP exchange are out of scope:
they are injected as callables, exactly where the reference's tests mock them
(OutputDeliveryServiceTest.java:183-209).
"""
from __future__ import annotations

import hashlib
import uuid
from typing import Callable, List, Sequence

import numpy as np

from . import _lib
from .client import pack, unpack
from .entities import (AmphoraServiceException, FactorPair, IllegalArgumentException,
                       MaskedInput, MultiplicationExchangeObject, OutputDeliveryObject,
                       SecretShare, SHARE_WIDTH, WORD_WIDTH)

INPUT_MASK_GFP = "INPUT_MASK_GFP"  # castor TupleType; tuple = value(16) || mac(16)
MULTIPLICATION_TRIPLE_GFP = "MULTIPLICATION_TRIPLE_GFP"  # a,mac,b,mac,c,mac (96 B)
TUPLE_SIZE = {INPUT_MASK_GFP: 32, MULTIPLICATION_TRIPLE_GFP: 96}


def name_uuid_from_bytes(name: bytes) -> uuid.UUID:
    """java.util.UUID.nameUUIDFromBytes (MD5, version 3)."""
    h = bytearray(hashlib.md5(name).digest())
    h[6] = (h[6] & 0x0F) | 0x30
    h[8] = (h[8] & 0x3F) | 0x80
    return uuid.UUID(bytes=bytes(h))


class SecretShareUtil:
    """Service-side SecretShareUtil (constructed from the SPDZ context)."""

    def __init__(self, ctx: _lib.Context):
        self._ctx = ctx

    def convert_to_secret_share(self, masked_input: MaskedInput, mac_key: str, input_masks,
                                use_zero_input_as_data: bool) -> SecretShare:
        """convertToSecretShare :58-81.  input_masks: the tuple stream
        (W x 32 B: share-0 value || mac) or a list of (value, mac) pairs."""
        masks = _tuples(input_masks, 32)
        if len(masked_input.data) != masks.shape[0]:
            raise IllegalArgumentException("Received more input data than available inputMasks.")
        data = masked_input.data
        if hasattr(data, "words"):  # MaskedInputWords: the array itself
            masked = data.words
        else:
            masked = np.frombuffer(b"".join(d.value for d in data), np.uint8).reshape(-1, 16) \
                if data else np.zeros((0, 16), np.uint8)
        key = int(mac_key) % self._ctx.prime  # new BigInteger(mac) :86 (used mod p)
        out = self._ctx.convert_share(masked, masks, key, use_zero_input_as_data)
        return SecretShare(masked_input.secret_id, out.tobytes(), list(masked_input.tags))

    def convert_masked_input_json(self, body, mac_key: str, input_masks,
                                  use_zero_input_as_data: bool) -> SecretShare:
        """POST /masked-inputs on the body text (MaskedInputController.upload ->
        StorageService.createSecret -> convertToSecretShare :58-107): when the
        "data" array is in Jackson's compact layout with one record per input
        mask, one launch (amph_convert_share_json) checks, decodes and converts
        it and only the small remainder of the body goes through json.loads.
        Any other body -- another legal layout, a record count other than the
        mask count, a byte the kernel refuses -- takes
        wire.masked_input_from_json + convert_to_secret_share, so it gets the
        reference's verdict and message."""
        from . import wire
        masks = _tuples(input_masks, 32)
        raw = body.encode("utf-8") if isinstance(body, str) else bytes(body)
        span = wire.masked_input_data_span(raw)
        if span is not None:
            lb, rb, rest = span
            if rb + 1 - lb == (37 * masks.shape[0] + 1 if masks.shape[0] else 2):
                try:
                    out = self._ctx.convert_share_json(raw[lb:rb + 1], masks, int(mac_key) % self._ctx.prime,
                                                       use_zero_input_as_data)
                except _lib.AmphoraNativeError as e:
                    if e.status not in (_lib.AMPH_E_LEN, _lib.AMPH_E_PARAM):
                        raise
                    out = None
                if out is not None:
                    import json
                    obj = json.loads(rest)
                    if obj.get("secretId") is None:
                        raise IllegalArgumentException("secretId is marked non-null but is null")
                    return SecretShare(uuid.UUID(obj["secretId"]), out.tobytes(), list(obj.get("tags") or []))
        mi = wire.masked_input_from_json(self._ctx, raw.decode("utf-8"))
        return self.convert_to_secret_share(mi, mac_key, input_masks, use_zero_input_as_data)

    def convert_masked_inputs_json(self, bodies, mac_key: str, list_of_input_masks,
                                   use_zero_input_as_data: bool) -> list:
        """convert_masked_input_json for K uploads in one launch
        (amph_convert_share_json_batch): one entry per upload, the SecretShare
        or the exception convert_masked_input_json raises for that upload.
        Bodies whose "data" span is compact with one record per input mask go
        through the one batch call; every other body -- another layout,
        another count, a byte the kernel refuses -- takes
        convert_masked_input_json itself and so keeps the reference's verdict
        and message."""
        import json
        from . import wire
        from .client import _outcome
        if len(bodies) != len(list_of_input_masks):
            raise ValueError("one list of input masks per body")
        K = len(bodies)
        out, parsed = [None] * K, {}
        for o in range(K):
            try:
                masks = _tuples(list_of_input_masks[o], 32)
                raw = bodies[o].encode("utf-8") if isinstance(bodies[o], str) else bytes(bodies[o])
                span = wire.masked_input_data_span(raw)
            except Exception:  # the single function raises it again as this upload's own
                continue
            if span is not None and span[1] + 1 - span[0] == _lib.masked_input_data_chars(masks.shape[0]):
                parsed[o] = (raw[span[0]:span[1] + 1], masks, span[2])
        idx = sorted(parsed)
        if idx:
            shares, bad = self._ctx.convert_share_json_batch([parsed[o][0] for o in idx],
                                                             [parsed[o][1] for o in idx],
                                                             int(mac_key) % self._ctx.prime, use_zero_input_as_data)

            def finish(rest, share):
                obj = json.loads(rest)
                if obj.get("secretId") is None:
                    raise IllegalArgumentException("secretId is marked non-null but is null")
                return SecretShare(uuid.UUID(obj["secretId"]), share.tobytes(), list(obj.get("tags") or []))

            for k, o in enumerate(idx):
                if bad[k] < 0:
                    out[o] = _outcome(finish, parsed[o][2], shares[k])
                else:
                    del parsed[o]
        for o in range(K):
            if o not in parsed:
                out[o] = _outcome(self.convert_masked_input_json, bodies[o], mac_key, list_of_input_masks[o],
                                  use_zero_input_as_data)
        return out


def _tuples(x, size):
    if isinstance(x, (list, tuple)):
        x = b"".join(bytes(a) + bytes(b) for a, b in x) if x and isinstance(x[0], tuple) else b"".join(x)
    return _lib.words_view(x, size)


def encode_diffs(pairs: Sequence[FactorPair]):
    """FactorPair list (signed BigIntegers, |x| < 2^128) -> (mag, neg) arrays."""
    mags, negs = bytearray(), bytearray()
    for fp in pairs:
        for x in (fp.a, fp.b):
            mags += abs(int(x)).to_bytes(16, "little")
            negs.append(1 if x < 0 else 0)
    n = len(pairs)
    return (np.frombuffer(bytes(mags), np.uint8).reshape(n, 2, 16).copy(),
            np.frombuffer(bytes(negs), np.uint8).reshape(n, 2).copy())


def decode_diffs(mag, neg) -> List[FactorPair]:
    vals = unpack(np.ascontiguousarray(mag).reshape(-1, 16))
    sg = np.ascontiguousarray(neg).reshape(-1).tolist()
    signed = [-v if s else v for v, s in zip(vals, sg)]
    return [FactorPair(signed[2 * k], signed[2 * k + 1]) for k in range(len(signed) // 2)]


def _check_partner(m, own):
    """A partner must open exactly as many FactorPairs as this party did: the
    reference's recombineDiffs reads every partner's list at each own index
    (:231-272) and fails inside the open's Try on a short one."""
    if tuple(m.shape) != tuple(own.shape):
        raise ValueError("partner opened %d pairs, expected %d" % (m.shape[0], own.shape[0]))


class OutputDeliveryService:
    """OutputDeliveryService with Castor and the inter-VCP open injected.

    tuple_source(request_id, tuple_type, count) -> bytes   (Castor download)
    exchange(MultiplicationExchangeObject) -> list of the partners' FactorPair
        lists in player order (open + Redis gather, recombineDiffs :231-272)

    exchange_format="json": the exchange carries the MultiplicationExchangeObject
    as its /inter-vcp/open JSON body (bytes in, partners' bodies out), coded on
    the GPU (amph_exchange_*) -- no per-value Python objects.
    exchange_format="session": the same JSON bodies, with the request run as a
    device-resident party session (amph_party_*): the triples and every party's
    diffs stay on the GPU between the open's two halves (needs n_parties).
    exchange_format="session_batch": the same bodies again, with ALL the live
    requests of a call run as ONE device-resident batch session
    (amph_parties_*, include/amphora_party_batch.h): a fixed number of
    launches whatever the request count, one verdict per request; the
    single-request functions run a batch of one (needs n_parties).
    """

    def __init__(self, ctx: _lib.Context, player_id: int,
                 tuple_source: Callable[[uuid.UUID, str, int], bytes],
                 exchange: Callable, exchange_format: str = "objects", n_parties: int = None):
        if exchange_format not in ("objects", "json", "session", "session_batch"):
            raise ValueError("exchange_format must be 'objects', 'json', 'session' or 'session_batch'")
        if exchange_format in ("session", "session_batch") and not n_parties:
            raise ValueError("exchange_format='%s' needs n_parties" % exchange_format)
        self._ctx = ctx
        self.player_id = player_id
        self._tuples = tuple_source
        self._exchange = exchange
        self._json = exchange_format == "json"
        self._session = exchange_format == "session"
        self._session_batch = exchange_format == "session_batch"
        self.n_parties = n_parties
        self.last_exchange_object = None

    def _download(self, request_id, tuple_type, count):
        try:
            data = self._tuples(request_id, tuple_type, count)
        except Exception as e:  # Try.of(..).getOrElseThrow :103-107, :178-185
            raise AmphoraServiceException("Failed to retrieve the required Tuples form Castor") from e
        try:
            tuples = _lib.words_view(data, TUPLE_SIZE[tuple_type])
        except ValueError as e:
            raise AmphoraServiceException("Castor returned a malformed %s stream" % tuple_type) from e
        if tuples.shape[0] != count:
            # the reference indexes tripleShares.get(i) / inputMasks.get(2i+1) and
            # fails with IndexOutOfBounds on a short list (:121-139, :186-200); the
            # kernels take one word count and cannot see a short buffer, so the
            # stream's length is checked before any launch
            raise AmphoraServiceException("Castor returned %d %s tuples, %d requested"
                                          % (tuples.shape[0], tuple_type, count))
        return tuples

    def compute_output_delivery_object(self, share, request_id: uuid.UUID) -> OutputDeliveryObject:
        """computeOutputDeliveryObject(SecretShare | byte[], UUID) :75-161."""
        if isinstance(share, SecretShare):
            data, stride = share.data, SHARE_WIDTH  # MACs stripped inside K_ODO_PRE (:79-84)
        else:
            data, stride = bytes(share), WORD_WIDTH
        return self._compute(_lib.words_view(data, stride), stride, request_id)

    def _open(self, op_id, mag, neg):
        """The inter-VCP open of one request: this party's diffs out, every
        party's (own first) back as (mags, negs)."""
        mags, negs = [mag], [neg]
        if self._json:
            from . import wire
            own = wire.exchange_to_json(self._ctx, op_id, self.player_id, mag, neg)
            self.last_exchange_object = own
            try:
                partners = self._exchange(own)
                for body in partners:
                    p_op, _, m, n = wire.exchange_from_json(self._ctx, body, mag.shape[0])
                    if p_op != op_id:
                        raise ValueError("operation id %s != %s" % (p_op, op_id))
                    _check_partner(m, mag)
                    mags.append(m)
                    negs.append(n)
            except Exception as e:
                raise AmphoraServiceException("Failed to open values for operation #%s" % op_id) from e
        else:
            xo = MultiplicationExchangeObject(op_id, self.player_id, decode_diffs(mag, neg))
            self.last_exchange_object = xo
            try:
                partners = self._exchange(xo)
                for lst in partners:  # recombineDiffs runs inside the same Try (:205-219)
                    m, n = encode_diffs(lst)
                    _check_partner(m, mag)
                    mags.append(m)
                    negs.append(n)
            except Exception as e:
                raise AmphoraServiceException("Failed to open values for operation #%s" % op_id) from e
        return mags, negs

    def _open_many(self, reqs, out):
        """_open (exchange_format="json") for many requests: reqs = {o: (op_id,
        mag, neg)}.  One batch encode writes every request's body, the exchange
        callback runs once per request (the protocol is per operation id), one
        batch decode parses every partner body of every request -- the objects
        in partner-major order.  Returns {o: (mags, negs)} as _open's; a request
        whose exchange, partner body or operation id fails gets out[o] = the
        AmphoraServiceException _open raises, and the others are unaffected."""
        from . import wire
        order = sorted(reqs)
        bodies = wire.exchange_bodies_to_json(self._ctx, [reqs[o][0] for o in order], self.player_id,
                                              [reqs[o][1] for o in order], [reqs[o][2] for o in order])
        partners, failed = {}, {}
        for o, own in zip(order, bodies):
            self.last_exchange_object = own
            try:
                partners[o] = list(self._exchange(own))
            except Exception as e:  # noqa: BLE001 -- this request's own outcome
                failed[o] = e
        items = [(j, o) for j in range(max([len(p) for p in partners.values()] or [0]))
                 for o in order if o in partners and j < len(partners[o])]
        got = wire.exchange_bodies_from_json(self._ctx, [partners[o][j] for j, o in items],
                                             [reqs[o][1].shape[0] for _, o in items])
        opened = {o: ([reqs[o][1]], [reqs[o][2]]) for o in partners}
        for (j, o), res in zip(items, got):
            if o in failed:
                continue
            if isinstance(res, Exception):
                failed[o] = res
            elif res[0] != reqs[o][0]:
                failed[o] = ValueError("operation id %s != %s" % (res[0], reqs[o][0]))
            else:
                _check_partner(res[2], reqs[o][1])  # (the decode's pair count fixes the shape: as _open, for the record)
                opened[o][0].append(res[2])
                opened[o][1].append(res[3])
        for o, e in failed.items():
            opened.pop(o, None)
            try:
                raise AmphoraServiceException("Failed to open values for operation #%s" % reqs[o][0]) from e
            except AmphoraServiceException as x:
                out[o] = x
        return opened

    def _compute(self, share_words, stride, request_id):
        if self._session_batch:  # a batch of one
            res = self._compute_many([share_words], stride, [request_id])[0]
            if isinstance(res, Exception):
                raise res
            return res
        W = share_words.shape[0]
        masks = self._download(request_id, INPUT_MASK_GFP, 2 * W)
        op_id = name_uuid_from_bytes(("%s_%d" % (request_id, 2 * W)).encode())  # :140-141
        triples = self._download(op_id, MULTIPLICATION_TRIPLE_GFP, 2 * W)
        if self._session:
            return self._compute_session(share_words, stride, masks, triples, op_id)
        y, r, v, mag, neg = self._ctx.odo_pre(share_words, stride, masks, triples)
        mags, negs = self._open(op_id, mag, neg)
        # recombineDiffs (:231-272) + multiplySharedSecrets (:274-286) + the w/u
        # encoding (:147-152), one launch: the opened values stay on chip
        w, u = self._ctx.open_post(mags, negs, triples, self.player_id == 0)
        return OutputDeliveryObject(y.tobytes(), r.tobytes(), v.tobytes(), w.tobytes(), u.tobytes())

    def _compute_session(self, share_words, stride, masks, triples, op_id):
        """_compute with the tuples, diffs and ODO fields device-resident
        (amph_party_begin -> the own body -> each partner's interimValues ->
        amph_party_finish); same results, bit for bit."""
        from . import wire
        with self._ctx.party_begin(share_words, stride, masks, triples, self.n_parties) as s:
            own = wire.exchange_body(op_id, self.player_id, s.text())
            self.last_exchange_object = own
            try:
                partners = self._exchange(own)
                if len(partners) != self.n_parties - 1:
                    raise ValueError("%d partner bodies, %d expected" % (len(partners), self.n_parties - 1))
                for slot, body in enumerate(partners, start=1):
                    body = bytes(body)
                    p_op, _, lb, rb = wire.exchange_span(body)
                    if p_op != op_id:
                        raise ValueError("operation id %s != %s" % (p_op, op_id))
                    s.partner(slot, body[lb:rb + 1])
            except Exception as e:
                raise AmphoraServiceException("Failed to open values for operation #%s" % op_id) from e
            w, u = s.finish(self.player_id == 0)
            return OutputDeliveryObject(s.y.tobytes(), s.r.tobytes(), s.v.tobytes(), w.tobytes(), u.tobytes())

    def get_input_masks_as_output_delivery_object(self, request_id: uuid.UUID, count: int):
        """InputMaskCachingService.getInputMasksAsOutputDeliveryObject :77-99:
        the mask tuples' value halves (stride 32) feed the ODO computation
        under odoRequestId = nameUUIDFromBytes(requestId + "_odo-computation").
        Returns (ODO, the mask tuple stream to cache)."""
        masks = self._download(request_id, INPUT_MASK_GFP, count)
        odo_req = name_uuid_from_bytes(("%s_odo-computation" % request_id).encode())
        return self._compute(masks, 32, odo_req), masks

    # -- K requests at once ------------------------------------------------------------
    def compute_output_delivery_objects(self, shares, request_ids) -> list:
        """compute_output_delivery_object for K requests: the tuple downloads
        and the exchange stay per request (they are the protocol's own), one
        K_ODO_PRE and one open + K_ODO_POST launch run over the concatenation of
        the requests' words -- both are word by word, so every request's ODO is
        bit for bit the single function's.  With exchange_format="json" the
        requests' bodies are written by one batch encode and all their
        partners' bodies parsed by one batch decode (_open_many).  Returns one entry per request: the
        OutputDeliveryObject, or the AmphoraServiceException the single function
        raises for that request (the others are unaffected).
        exchange_format="session" is one request by construction: a loop;
        "session_batch" runs the live requests as one batch session
        (_compute_many_session)."""
        if len(shares) != len(request_ids):
            raise ValueError("one request id per share")
        if self._session:
            from .client import _outcome
            return [_outcome(self.compute_output_delivery_object, s, r) for s, r in zip(shares, request_ids)]
        views = [(_lib.words_view(s.data, SHARE_WIDTH), SHARE_WIDTH) if isinstance(s, SecretShare)
                 else (_lib.words_view(bytes(s), WORD_WIDTH), WORD_WIDTH) for s in shares]
        if len({st for _, st in views}) > 1:  # mixed: the value halves alone, which is all K_ODO_PRE reads
            views = [(np.ascontiguousarray(v[:, :WORD_WIDTH]), WORD_WIDTH) for v, _ in views]
        return self._compute_many([v for v, _ in views], views[0][1] if views else WORD_WIDTH, request_ids)

    def _compute_many(self, words, stride, request_ids) -> list:
        K = len(words)
        out, got = [None] * K, {}
        for o in range(K):
            W = words[o].shape[0]
            try:
                masks = self._download(request_ids[o], INPUT_MASK_GFP, 2 * W)
                op_id = name_uuid_from_bytes(("%s_%d" % (request_ids[o], 2 * W)).encode())
                got[o] = (masks, op_id, self._download(op_id, MULTIPLICATION_TRIPLE_GFP, 2 * W))
            except AmphoraServiceException as e:
                out[o] = e
        live = sorted(got)
        if not live:
            return out
        if self._session_batch:
            return self._compute_many_session(words, stride, got, out)
        at, off = 0, {}
        for o in live:
            off[o] = at
            at += words[o].shape[0]
        y, r, v, mag, neg = self._ctx.odo_pre(np.concatenate([words[o] for o in live]), stride,
                                              np.concatenate([got[o][0] for o in live]),
                                              np.concatenate([got[o][2] for o in live]))
        opened = {}
        cut = {o: (2 * off[o], 2 * (off[o] + words[o].shape[0])) for o in live}
        if self._json:  # one encode and one decode call for all the requests' bodies
            opened = self._open_many({o: (got[o][1], mag[a:b], neg[a:b]) for o, (a, b) in cut.items()}, out)
        else:
            for o in live:  # the exchange works on this request's slice of the packed diffs
                a, b = cut[o]
                try:
                    opened[o] = self._open(got[o][1], mag[a:b], neg[a:b])
                except AmphoraServiceException as e:
                    out[o] = e
        groups = {}  # by party count: one open + K_ODO_POST launch each (one group, unless a partner list is off)
        for o in sorted(opened):
            groups.setdefault(len(opened[o][0]), []).append(o)
        for n, members in groups.items():
            mags = [np.concatenate([opened[o][0][j] for o in members]) for j in range(n)]
            negs = [np.concatenate([opened[o][1][j] for o in members]) for j in range(n)]
            w, u = self._ctx.open_post(mags, negs, np.concatenate([got[o][2] for o in members]), self.player_id == 0)
            g0 = 0
            for o in members:
                a, W = off[o], words[o].shape[0]
                out[o] = OutputDeliveryObject(y[a:a + W].tobytes(), r[a:a + W].tobytes(), v[a:a + W].tobytes(),
                                              w[g0:g0 + W].tobytes(), u[g0:g0 + W].tobytes())
                g0 += W
        return out

    def _compute_many_session(self, words, stride, got, out) -> list:
        """_compute_many's live requests (got = {o: (masks, op_id, triples)}) as
        ONE batch session: begin over the concatenation, the exchange callback
        per request on wire.exchange_body of its own text, every partner's K
        texts in one call per slot, one finish.  A request whose exchange
        fails, whose partner body carries another operation id or count, or
        whose partner text the decode refuses gets the AmphoraServiceException
        _compute_session raises for it; its slots are filled with an empty
        text, which the session rejects for that object alone."""
        from . import wire
        live = sorted(got)
        woff = np.concatenate([[0], np.cumsum([words[o].shape[0] for o in live])]).astype(np.uint64)
        n, failed = self.n_parties, {}
        with self._ctx.parties_begin(np.concatenate([words[o] for o in live]), stride,
                                     np.concatenate([got[o][0] for o in live]),
                                     np.concatenate([got[o][2] for o in live]), woff, n) as s:
            texts = [[b""] * len(live) for _ in range(n)]  # texts[slot][k]
            for k, (o, own_text) in enumerate(zip(live, s.texts())):
                op_id = got[o][1]
                own = wire.exchange_body(op_id, self.player_id, own_text)
                self.last_exchange_object = own
                try:
                    partners = self._exchange(own)
                    if len(partners) != n - 1:
                        raise ValueError("%d partner bodies, %d expected" % (len(partners), n - 1))
                    mine = []
                    for body in partners:
                        body = bytes(body)
                        p_op, _, lb, rb = wire.exchange_span(body)
                        if p_op != op_id:
                            raise ValueError("operation id %s != %s" % (p_op, op_id))
                        if rb + 1 - lb > _lib.exchange_slot_chars(2 * words[o].shape[0]):
                            raise ValueError("interimValues must hold exactly %d FactorPairs"
                                             % (2 * words[o].shape[0]))  # (longer than any text of that many)
                        mine.append(body[lb:rb + 1])
                    for slot, t in enumerate(mine, start=1):
                        texts[slot][k] = t
                except Exception as e:  # noqa: BLE001 -- this request's own outcome
                    failed[o] = e
            for slot in range(1, n):
                bad, _ = s.partner(slot, texts[slot], status=True)
                for k, o in enumerate(live):
                    if bad[k] >= 0 and o not in failed:
                        P = 2 * words[o].shape[0]
                        failed[o] = ValueError("interimValues must hold exactly %d FactorPairs" % P
                                               if bad[k] == len(texts[slot][k])
                                               else "Malformed FactorPair JSON at offset %d" % bad[k])
            w, u = s.finish(self.player_id == 0)
            for k, o in enumerate(live):
                a, b = int(woff[k]), int(woff[k + 1])
                if o in failed:
                    try:
                        raise AmphoraServiceException("Failed to open values for operation #%s" % got[o][1]) \
                            from failed[o]
                    except AmphoraServiceException as x:
                        out[o] = x
                else:
                    out[o] = OutputDeliveryObject(s.y[a:b].tobytes(), s.r[a:b].tobytes(), s.v[a:b].tobytes(),
                                                  w[a:b].tobytes(), u[a:b].tobytes())
        return out

    def get_input_masks_as_output_delivery_objects(self, request_ids, counts) -> list:
        """get_input_masks_as_output_delivery_object for K requests over the
        stride-32 mask tuples, as compute_output_delivery_objects: one entry per
        request, (ODO, the mask tuple stream to cache) or the request's
        AmphoraServiceException."""
        if len(request_ids) != len(counts):
            raise ValueError("one count per request id")
        if self._session:
            from .client import _outcome
            return [_outcome(self.get_input_masks_as_output_delivery_object, r, c)
                    for r, c in zip(request_ids, counts)]
        out, masks = [None] * len(request_ids), {}
        for o, (rid, count) in enumerate(zip(request_ids, counts)):
            try:
                masks[o] = self._download(rid, INPUT_MASK_GFP, count)
            except AmphoraServiceException as e:
                out[o] = e
        live = sorted(masks)
        odo_reqs = [name_uuid_from_bytes(("%s_odo-computation" % request_ids[o]).encode()) for o in live]
        for o, res in zip(live, self._compute_many([masks[o] for o in live], 32, odo_reqs)):
            out[o] = res if isinstance(res, Exception) else (res, masks[o])
        return out
