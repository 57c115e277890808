"""The Input Supply upload on the MaskedInput JSON text, both ends
(amph_convert_share_json, amph_mask_input_json):

* party: POST /masked-inputs -> MaskedInputController.upload ->
  StorageService.createSecret -> service SecretShareUtil.convertToSecretShare
  (SecretShareUtil.java:58-107) on the "data" array text of the body
  (MaskedInput.java:25-62, MaskedInputData.java:44-52);
* client: DefaultAmphoraClient.createSecret :150-170 with the masked words
  written as that text.

Expected values come from the Python restatement of the reference
(oracle.amphora_oracle.convert_to_secret_share / create_secret_masked_inputs)
and Python's base64 / json.  T = 128 is the party kernel's words per
workgroup, 192 the mask kernel's."""
import base64
import ctypes as C
import json
import random
import uuid

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import amphora_oracle as O  # noqa: E402
from oracle import coracle  # noqa: E402

T = 128
NF = 0x7F7F7F7F7F7F7F7F
E_LEN, E_PARAM = 2, 3
F_DEVICE, F_HOST_IO = 1, 4
WMAX = 2 * T + 3
_SMALL = 2 ** 89 - 1
FIELDS = {"big": (O.TEST_PRIME, O.TEST_R, O.TEST_RINV),
          "small": (_SMALL, pow(2, 128, _SMALL), pow(pow(2, 128, _SMALL), -1, _SMALL))}


def data_text(words16) -> bytes:
    """Jackson's compact "data" array of the given 16-byte words."""
    return json.dumps([{"value": base64.b64encode(bytes(w)).decode()} for w in words16],
                      separators=(",", ":")).encode()


class Case:
    """One field kind: a context and, computed once, WMAX masked words, mask
    tuples, a MAC key and the oracle's shares for both use_zero values (the
    conversion is word by word, so a prefix of W words is the case for W)."""

    def __init__(self, kind):
        import torch
        assert torch.cuda.is_available()
        import amphora_amd as A
        self.p, self.r, self.rinv = FIELDS[kind]
        self.ctx = A.Context(self.p, self.r, self.rinv)
        self.spdz = O.MpSpdzIntegrationUtils(self.p, self.r, self.rinv)
        rng = random.Random(1234 + len(kind))
        self.key = rng.randrange(1, self.p)
        masked = [rng.randrange(self.p).to_bytes(16, "little") for _ in range(WMAX)]
        for i in range(0, WMAX, 3):  # records that encode values >= p (any 128-bit word is legal)
            masked[i] = masked[i][:15] + b"\xEE"
        masked[1] = b"\xFF" * 16
        assert int.from_bytes(masked[0], "little") >= self.p
        self.masked = masked
        self.tuples = [(rng.randrange(self.p).to_bytes(16, "little"), rng.randrange(self.p).to_bytes(16, "little"))
                       for _ in range(WMAX)]
        self.tup_bytes = b"".join(a + b for a, b in self.tuples)
        self.share = {uz: O.convert_to_secret_share(self.spdz, masked, str(self.key), self.tuples, uz)
                      for uz in (False, True)}

    def tup(self, W):
        return np.frombuffer(self.tup_bytes[:32 * W], np.uint8).reshape(W, 32)

    def text(self, W):
        return data_text(self.masked[:W])


@pytest.fixture(scope="module", params=["big", "small"])
def case(request):
    return Case(request.param)


def _abi():
    import amphora_amd as A
    return A._lib.lib


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.uint8)).cuda()  # (a writable copy)


def _text_dev(text: bytes, align: int = 0, pad: int = 48):
    """The text as a view at byte offset `align` of a 0xFF-filled device buffer."""
    import torch
    buf = torch.full((align + len(text) + pad,), 0xFF, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[align:align + len(text)]
    view.copy_(torch.frombuffer(bytearray(text), dtype=torch.uint8))
    return buf, view


def convert(case, text: bytes, W: int, uz: bool, mode: str, align: int = 0):
    """-> (share bytes, bad) with bad = -1 when clean (host: a refused text raises)."""
    if mode == "host":
        return case.ctx.convert_share_json(text, case.tup(W), case.key, uz).tobytes(), -1
    import torch
    _, view = _text_dev(text, align)
    out, bad = case.ctx.convert_share_json(view, _dev(case.tup(W)), case.key, uz)
    torch.cuda.synchronize()
    b = int(bad.item())
    return out.cpu().numpy().tobytes(), (-1 if b == NF else b)


# ---- 1. parity with the oracle ---------------------------------------------------
@pytest.mark.parametrize("mode", ["host", "device"])
@pytest.mark.parametrize("W", [0, 1, 2, 15, 16, 17, T - 1, T, T + 1, 2 * T + 3])
def test_convert_share_json_matches_oracle(case, mode, W):
    text = case.text(W)
    assert len(text) == _abi().amph_masked_input_data_chars(W) == (37 * W + 1 if W else 2)
    for uz in (False, True):
        share, bad = convert(case, text, W, uz, mode)
        assert bad == -1
        assert share == case.share[uz][:32 * W]
    if W and mode == "host":  # bit for bit what the two launches it replaces give
        rec = np.frombuffer(text[1:] if W else b"", np.uint8).reshape(W, 37)[:, 10:34]
        two = case.ctx.convert_share(case.ctx.base64_decode_words(np.ascontiguousarray(rec)), case.tup(W),
                                     case.key, False)
        assert two.tobytes() == case.share[False][:32 * W]


# ---- 2. text alignment ---------------------------------------------------------
@pytest.mark.parametrize("W", [17, T + 1])
def test_text_at_every_byte_alignment(case, W):
    import torch
    lib, text = _abi(), case.text(W)
    tup = _dev(case.tup(W))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for align in range(16):
        buf, view = _text_dev(text, align)
        assert view.data_ptr() % 16 == align
        out = torch.full((W + 4, 32), 0xA5, dtype=torch.uint8, device="cuda")  # guard rows: 2 before, 2 after
        bad = torch.zeros(1, dtype=torch.int64, device="cuda")
        st = lib.amph_convert_share_json(case.ctx._h, view.data_ptr(), len(text), W, tup.data_ptr(),
                                         case.key.to_bytes(16, "little"), 0, out[2:].data_ptr(),
                                         C.cast(C.c_void_p(bad.data_ptr()), C.POINTER(C.c_int64)), F_DEVICE, stream)
        torch.cuda.synchronize()
        assert st == 0 and int(bad.item()) == NF, align
        o = out.cpu().numpy()
        assert o[2:W + 2].tobytes() == case.share[False][:32 * W], align
        assert (o[:2] == 0xA5).all() and (o[W + 2:] == 0xA5).all(), align
        b = buf.cpu().numpy()  # (the text is only read)
        assert (b[:align] == 0xFF).all() and (b[align + len(text):] == 0xFF).all()


# ---- 3. rejections -----------------------------------------------------------------
def _alter(ch: int) -> int:
    return {ord(","): ord("]"), ord("]"): ord(",")}.get(ch, ch ^ 0x20)


def _rejections(W):
    """(offset in the text, replacement byte) of every single fault the issue
    lists, on a record of the first workgroup and on the last record."""
    out = []
    for rec in (5, W - 1):
        base = 1 + 37 * rec
        for c in (0, 15, 16, 21):  # a byte outside the alphabet
            out.append((base + 10 + c, b"*-\x80 "[c % 4]))
        out.append((base + 10 + 21, ord("=")))
        out.append((base + 10 + 22, ord("A")))
        out.append((base + 10 + 23, ord("A")))
        for k in list(range(10)) + [34, 35, 36]:  # the 13 frame bytes (36 of the last record: the final ']')
            out.append((base + k, None))
    out.append((0, None))  # the leading '['
    return out


def test_rejections_report_the_offending_byte(case):
    import torch
    W = T + 1
    text = case.text(W)
    tup = _dev(case.tup(W))
    cases = _rejections(W)
    assert (37 * W, None) in cases  # the final ']' -> ','
    for off, new in cases:
        t = bytearray(text)
        t[off] = _alter(t[off]) if new is None else new
        assert t[off] != text[off]
        _, view = _text_dev(bytes(t), align=off % 16)
        _, bad = case.ctx.convert_share_json(view, tup, case.key, False)
        assert int(bad.item()) == off, (off, new)
    # two faults: the smaller offset wins (across workgroups, either order in the text)
    for a, b in ((1 + 37 * 3 + 12, 1 + 37 * (W - 1) + 4), (1 + 37 * 100 + 36, 1 + 37 * 7 + 35)):
        t = bytearray(text)
        t[a] = t[b] = ord("!")
        _, bad = case.ctx.convert_share_json(_text_dev(bytes(t))[1], tup, case.key, False)
        assert int(bad.item()) == min(a, b)
    torch.cuda.synchronize()


def test_rejections_host_mode(case):
    import amphora_amd as A
    lib, W = _abi(), T + 1
    text = case.text(W)
    for off in (0, 1 + 37 * 5 + 10 + 21, 1 + 37 * 5 + 34, 1 + 37 * (W - 1) + 3, 37 * W):
        t = bytearray(text)
        t[off] = ord("=") if t[off] != ord("=") else ord("A")
        out = np.zeros((W, 32), np.uint8)
        bad = C.c_int64(-7)
        st = lib.amph_convert_share_json(case.ctx._h, bytes(t), len(t), W, case.tup(W).ctypes.data,
                                         case.key.to_bytes(16, "little"), 0, out.ctypes.data, C.byref(bad), 0, None)
        assert st == E_PARAM and bad.value == off
        msg = lib.amph_last_error().decode()
        assert "offset %d" % off in msg
        assert ("record %d" % ((off - 1) // 37) in msg) if off else ("'['" in msg)
        with pytest.raises(A.AmphoraNativeError, match="offset %d" % off):
            case.ctx.convert_share_json(bytes(t), case.tup(W), case.key, False)
    bad = C.c_int64(-7)
    out = np.zeros((W, 32), np.uint8)
    assert lib.amph_convert_share_json(case.ctx._h, text, len(text), W, case.tup(W).ctypes.data,
                                       case.key.to_bytes(16, "little"), 0, out.ctypes.data, C.byref(bad), 0,
                                       None) == 0 and bad.value == -1


@pytest.mark.parametrize("mode", ["host", "device"])
def test_wrong_length_and_host_io_are_refused(case, mode):
    import torch
    lib, W = _abi(), T + 1
    text = case.text(W)
    key = case.key.to_bytes(16, "little")
    pattern = np.arange(32 * W, dtype=np.uint32).astype(np.uint8).reshape(W, 32)
    if mode == "host":
        out, tup, txt, flags, stream = pattern.copy(), case.tup(W), np.frombuffer(text, np.uint8), 0, None
        ptr = lambda a: a.ctypes.data  # noqa: E731
        bad, badp = C.c_int64(-7), None
        badp = C.pointer(bad)
    else:
        out, tup, txt, flags = _dev(pattern), _dev(case.tup(W)), _text_dev(text)[1], F_DEVICE
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ptr = lambda a: a.data_ptr()  # noqa: E731
        bad = torch.full((1,), -7, dtype=torch.int64, device="cuda")
        badp = C.cast(C.c_void_p(bad.data_ptr()), C.POINTER(C.c_int64))
    for length, words in ((len(text) - 1, W), (len(text), W - 1), (len(text), W + 1), (2, W)):
        st = lib.amph_convert_share_json(case.ctx._h, ptr(txt), length, words, ptr(tup), key, 0, ptr(out), badp,
                                         flags, stream)
        assert st == E_LEN, (length, words)
        if mode == "device":
            torch.cuda.synchronize()
        got = out if mode == "host" else out.cpu().numpy()
        assert np.array_equal(got, pattern)  # nothing launched, nothing written
    st = lib.amph_convert_share_json(case.ctx._h, ptr(txt), len(text), W, ptr(tup), key, 0, ptr(out), badp,
                                     F_HOST_IO, stream)
    assert st == E_PARAM
    got = out if mode == "host" else out.cpu().numpy()
    assert np.array_equal(got, pattern)


# ---- 4. service and loopback ---------------------------------------------------
def _body(case, W, tags, pretty=False, values=None):
    sid = uuid.UUID("80fbba1b-3da8-4b1e-8a2c-cebd65229fad")
    vals = values if values is not None else [base64.b64encode(w).decode() for w in case.masked[:W]]
    obj = {"secretId": str(sid), "data": [{"value": v} for v in vals], "tags": tags}
    return json.dumps(obj, indent=2) if pretty else json.dumps(obj, separators=(",", ":"))


def test_service_convert_masked_input_json(case):
    from amphora_amd import entities as E
    from amphora_amd import wire
    from amphora_amd.service import SecretShareUtil
    util, W = SecretShareUtil(case.ctx), T + 1
    tags = [{"key": "k", "value": "v", "valueType": "STRING"}]
    tricky = [{"key": '"data":[', "value": 'x"data":[{"value":"]', "valueType": "STRING"}]

    def reference(body, uz):
        return util.convert_to_secret_share(wire.masked_input_from_json(case.ctx, body), str(case.key),
                                            case.tup(W), uz)

    for body, fused in ((_body(case, W, tags), True), (_body(case, W, tags, pretty=True), False),
                        (_body(case, W, tricky), None)):
        for uz in (False, True):
            before = case.ctx.stats()["kernel_launches"]
            got = util.convert_masked_input_json(body, str(case.key), case.tup(W), uz)
            launches = case.ctx.stats()["kernel_launches"] - before
            exp = reference(body, uz)
            assert got.data == exp.data == case.share[uz][:32 * W]
            assert got.secret_id == exp.secret_id and got.tags == exp.tags
            if fused is not None:  # one launch on the text; the decode's and the conversion's through the fallback
                assert (launches == 1) if fused else (launches >= 2), launches
    # bytes in, and no words at all
    assert util.convert_masked_input_json(_body(case, W, tags).encode(), str(case.key), case.tup(W),
                                          False).data == case.share[False][:32 * W]
    assert util.convert_masked_input_json(_body(case, 0, tags), str(case.key), case.tup(0), False).data == b""
    # the reference's verdicts on bodies the fused call does not take
    short = [base64.b64encode(w).decode() for w in case.masked[:W]]
    short[3] = short[3][:20]
    with pytest.raises(E.IllegalArgumentException, match="Length of a Masked Input value has to be 16 bytes."):
        util.convert_masked_input_json(_body(case, W, tags, values=short), str(case.key), case.tup(W), False)
    for masks in (case.tup(W - 1), case.tup(W + 1)):
        with pytest.raises(E.IllegalArgumentException, match="Received more input data than available inputMasks."):
            util.convert_masked_input_json(_body(case, W, tags), str(case.key), masks, False)
    # a refused character in a compact body: the fallback's (the codec's) verdict
    bad = _body(case, W, tags).replace('"value":"', '"value":"*', 1).replace('=="}', '="}', 1)
    with pytest.raises(ValueError):
        util.convert_masked_input_json(bad, str(case.key), case.tup(W), False)


@pytest.mark.parametrize("n,W", [(2, 1000), (3, 33)])
def test_loopback_wire_transport(n, W):
    import amphora_amd as A
    from amphora_amd.loopback import AmphoraParty, ExchangeHub, LoopbackAmphoraClient
    from tests.loopback_dealer import FakeCastor
    P, R, RINV = FIELDS["big"]
    spdz = O.MpSpdzIntegrationUtils(P, R, RINV)
    rng = random.Random(W + n)
    keys = [rng.randrange(P) for _ in range(n)]
    castor = FakeCastor(P, R, RINV, keys, W + n)
    hub = ExchangeHub(n)
    parties = [AmphoraParty(j, P, R, RINV, keys[j], castor, hub) for j in range(n)]
    client = LoopbackAmphoraClient(parties, P, R, RINV, transport="wire")
    data = [rng.randrange(2 ** 63) if i % 2 else rng.randrange(P) for i in range(W)]
    before = [p.ctx.stats()["kernel_launches"] for p in parties]
    sid = client.create_secret(A.Secret.of([("k", "v")], data))
    assert all(sid in p.secrets and not p.input_mask_store for p in parties)
    got = client.get_secret(sid)
    assert got.data == data
    alpha = sum(keys) % P
    for i in range(W):
        val = sum(spdz.from_gfp(p.secrets[sid].data[32 * i:32 * i + 16]) for p in parties) % P
        mac = sum(spdz.from_gfp(p.secrets[sid].data[32 * i + 16:32 * i + 32]) for p in parties) % P
        assert val == data[i] % P and mac == alpha * val % P
    assert all(p.ctx.stats()["kernel_launches"] > b for p, b in zip(parties, before))
    client.close()


# ---- client side ---------------------------------------------------------------
_CLIENT_FIELDS = {}


def _client_field(kind):
    if kind not in _CLIENT_FIELDS:
        import amphora_amd as A
        _CLIENT_FIELDS[kind] = (A.Context(*FIELDS[kind]), coracle.Field(*FIELDS[kind], threads=8))
    return _CLIENT_FIELDS[kind]


class ClientCase:
    """N parties' honest Input Mask ODOs (W words), S secrets and the oracle's
    masked words, for the big field (the small one where asked)."""

    def __init__(self, n, S, W, kind="big", fault=-1):
        self.p, r, rinv = FIELDS[kind]
        self.ctx, Fd = _client_field(kind)
        self.n, self.S, self.W = n, S, W
        self.odos, _ = Fd.synth_odos(seed=3000 + 7 * n + S, n=n, W=W, noncanon_permille=20, fault_index=fault)
        rng = random.Random(S + n)
        self.secrets = [rng.randrange(self.p) for _ in range(S)]
        self.sec16 = np.frombuffer(b"".join(s.to_bytes(16, "little") for s in self.secrets), np.uint8).reshape(S, 16)
        self.texts = [[base64.b64encode(np.ascontiguousarray(f).tobytes()) for f in o] for o in self.odos]
        self.util = O.ClientSecretShareUtil(self.p, r, rinv)

    def oracle_masked(self):
        odos = [O.OutputDeliveryObject(*[np.ascontiguousarray(f).tobytes() for f in o]) for o in self.odos]
        return O.create_secret_masked_inputs(self.util, self.secrets, odos)

    def dev_texts(self):
        import torch
        return [[torch.frombuffer(bytearray(t), dtype=torch.uint8).cuda() for t in o] for o in self.texts]


@pytest.mark.parametrize("mode", ["host", "device"])
@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("S,W", [(0, 1), (1, 1), (2, 9), (191, 191), (192, 192), (193, 200), (2 * 192 + 5, 2 * 192 + 5),
                                 (2 * 192 + 5, 3 * 192 + 1)])
def test_mask_input_json_text(mode, n, S, W):
    import torch
    c = ClientCase(n, S, W)
    exp = data_text(c.oracle_masked())
    assert len(exp) == (37 * S + 1 if S else 2)
    if mode == "host":
        text, ff, bad = c.ctx.mask_input_json(c.texts, W, c.sec16)
        assert ff == -1 and bad == -1 and text == exp
        return
    text, ff, bad = c.ctx.mask_input_json(c.dev_texts(), W, _dev(c.sec16))
    torch.cuda.synchronize()
    assert int(ff.item()) == NF and int(bad.item()) == NF
    assert text.cpu().numpy().tobytes() == exp


@pytest.mark.parametrize("mode", ["host", "device"])
@pytest.mark.parametrize("S,W", [(0, 3), (1, 1), (192, 192), (193, 193), (389, 400)])
def test_mask_input_json_capacity_and_guard_bytes(mode, S, W):
    import torch
    lib = _abi()
    c = ClientCase(2, S, W)
    exp = data_text(c.oracle_masked())
    chars = len(exp)
    ff, bad = C.c_int64(-7), C.c_int64(-7)
    if mode == "host":
        arr, keep = c.ctx._text_structs(c.texts)
        out = np.full(chars + 64, 0xFF, np.uint8)
        args = (c.sec16.ctypes.data, S, out.ctypes.data)
        tail = (C.byref(ff), C.byref(bad), 0, None)
    else:
        arr, keep = c.ctx._text_structs(c.dev_texts())
        sec, out = _dev(c.sec16), torch.full((chars + 64,), 0xFF, dtype=torch.uint8, device="cuda")
        v = torch.zeros(2, dtype=torch.int64, device="cuda")
        args = (sec.data_ptr(), S, out.data_ptr())
        tail = (C.cast(C.c_void_p(v.data_ptr()), C.POINTER(C.c_int64)),
                C.cast(C.c_void_p(v.data_ptr() + 8), C.POINTER(C.c_int64)), F_DEVICE,
                C.c_void_p(torch.cuda.current_stream().cuda_stream))
    host = lambda: out if mode == "host" else out.cpu().numpy()  # noqa: E731
    assert lib.amph_mask_input_json(c.ctx._h, arr, 2, W, *args, chars - 1, *tail) == E_LEN
    assert (host() == 0xFF).all()  # too small a capacity: nothing written
    assert lib.amph_mask_input_json(c.ctx._h, arr, 2, W, *args, chars, *tail) == 0
    if mode == "device":
        torch.cuda.synchronize()
    got = host()
    assert got[:chars].tobytes() == exp
    assert (got[chars:] == 0xFF).all()  # nothing past the ']'


@pytest.mark.parametrize("mode", ["host", "device"])
def test_mask_input_json_verdicts_equal_mask_input_b64(mode):
    """The same inputs to both calls: status (or exception), first_fail and
    bad_char must agree -- MAC fault, bad character, more secrets than masks."""
    import torch

    def both(c, texts, W, sec):
        res = []
        for fn in (lambda: c.ctx.mask_input_b64(texts, W, sec, records=True)[2:],
                   lambda: c.ctx.mask_input_json(texts, W, sec)[1:]):
            try:
                ff, bad = fn()
                if mode == "device":
                    torch.cuda.synchronize()
                    ff, bad = int(ff.item()), int(bad.item())
                res.append(("ok", ff, bad))
            except Exception as e:  # noqa: BLE001 -- compared below
                res.append((type(e).__name__, getattr(e, "status", None), str(e)))
        assert res[0] == res[1], res
        return res[0]

    prep = (lambda c: (c.texts, c.sec16)) if mode == "host" else (lambda c: (c.dev_texts(), _dev(c.sec16)))
    none = -1 if mode == "host" else NF
    # a MAC fault inside and past the secrets
    for S, W, fault in ((200, 300, 150), (200, 300, 299), (389, 389, 0)):
        c = ClientCase(3, S, W, fault=fault)
        texts, sec = prep(c)
        assert both(c, texts, W, sec) == ("ok", fault, none)
    # a character outside the alphabet (party 1's r field), alone and with a MAC fault
    for fault in (-1, 7):
        c = ClientCase(2, 200, 200, fault=fault)
        t = bytearray(c.texts[1][1])
        t[1000] = ord("*")
        c.texts[1][1] = bytes(t)
        texts, sec = prep(c)
        r = both(c, texts, 200, sec)
        nchars = len(t)
        if mode == "host":
            assert r[0] == "ValueError" and "index 1000 of party 1" in r[2]
        else:
            assert r[0] == "ok" and r[2] == (5 * 1 + 1) * nchars + 1000
    # more secrets than masks: every mask is verified first (a MAC fault is the
    # verdict), and only then the length error; device mode waits for the verdicts
    for fault in (-1, 3):
        c = ClientCase(2, 10, 8, fault=fault)
        texts, sec = prep(c)
        r = both(c, texts, 8, sec)
        assert (r[:2] == ("AmphoraNativeError", E_LEN)) if fault < 0 else (r == ("ok", fault, none)), r


@pytest.mark.parametrize("kind,n", [("big", 1), ("big", 2), ("big", 3), ("small", 3)])
def test_client_text_feeds_the_parties(kind, n):
    """createSecret's text -> each of 2 parties' convert_share_json -> the
    oracle's shares of the oracle's masked words."""
    S, W = 2 * 192 + 5, 2 * 192 + 5
    c = ClientCase(n, S, W, kind=kind)
    text, ff, bad = c.ctx.mask_input_json(c.texts, W, c.sec16)
    assert ff == -1 and bad == -1
    masked = c.oracle_masked()
    assert text == data_text(masked)
    spdz = O.MpSpdzIntegrationUtils(*FIELDS[kind])
    rng = random.Random(n)
    for party in range(2):
        key = rng.randrange(1, c.p)
        tuples = [(rng.randrange(c.p).to_bytes(16, "little"), rng.randrange(c.p).to_bytes(16, "little"))
                  for _ in range(S)]
        exp = O.convert_to_secret_share(spdz, masked, str(key), tuples, party != 0)
        tup = np.frombuffer(b"".join(a + b for a, b in tuples), np.uint8).reshape(S, 32)
        assert c.ctx.convert_share_json(text, tup, key, party != 0).tobytes() == exp
