"""Many MaskedInput uploads per launch, both ends
(include/amphora_upload_batch.h: amph_convert_share_json_packed / _batch,
amph_mask_input_json_packed / _batch).

Expected values come from the Python restatement of the reference
(oracle.amphora_oracle.convert_to_secret_share / create_secret_masked_inputs)
and Python's base64 / json (data_text, restated here); every object is also
compared with the library's single call on that object alone.  128 is the
party kernel's words per workgroup, 192 the mask kernel's; the size lists hold
both edges of each, empty objects first and in the middle, and more than one
tile per object.  (The copy-count test alone takes its expected masked words
from the C restatement oracle/coracle: 12,800 words.)"""
import base64
import ctypes as C
import functools
import json
import random
import uuid

import numpy as np
import pytest

from oracle import amphora_oracle as O
from oracle import coracle
from tests import extent_cases as X

pytestmark = pytest.mark.gpu

NF = 0x7F7F7F7F7F7F7F7F
OK, E_VERIFY, E_PARAM = 0, 1, 3
F_DEVICE = 1
_SMALL = 2 ** 89 - 1
FIELDS = {"big": (O.TEST_PRIME, O.TEST_R, O.TEST_RINV),
          "small": (_SMALL, pow(2, 128, _SMALL), pow(pow(2, 128, _SMALL), -1, _SMALL))}
CONV_SIZES = [0, 1, 2, 127, 128, 129, 0, 257, 1]  # t = 128
MASK_SIZES = [0, 1, 191, 192, 193, 0, 385]        # t = 192
MODES = ["host_packed", "host_batch", "device_packed"]


def data_text(words16) -> bytes:
    """Jackson's compact "data" array of the given 16-byte words."""
    return json.dumps([{"value": base64.b64encode(bytes(w)).decode()} for w in words16],
                      separators=(",", ":")).encode()


def data_chars(W):
    return 37 * W + 1 if W else 2


def nchars_of(W):
    return 4 * ((16 * W + 2) // 3)


def offsets_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)


def _dev(x):
    import torch
    x = np.array(x, copy=True)
    return torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).cuda()


def _host(v):
    import torch
    torch.cuda.synchronize()
    v = v.cpu().numpy()
    return np.where(v == NF, -1, v) if v.dtype == np.int64 else v


@functools.lru_cache(maxsize=None)
def _ctx(kind):
    import amphora_amd as A
    return A.Context(*FIELDS[kind])


# ================================================================= party side
class ConvCase:
    """One field kind: WMAX masked words, tuples, a MAC key and the oracle's
    shares for both use_zero values, computed once (the conversion is word by
    word: rows [a, b) are the case of the object holding words [a, b))."""
    WMAX = sum(CONV_SIZES)

    def __init__(self, kind):
        self.kind = kind
        self.p, self.r, self.rinv = FIELDS[kind]
        self.ctx = _ctx(kind)
        spdz = O.MpSpdzIntegrationUtils(self.p, self.r, self.rinv)
        rng = random.Random(4321 + len(kind))
        self.key = rng.randrange(1, self.p)
        masked = [rng.randrange(self.p).to_bytes(16, "little") for _ in range(self.WMAX)]
        for i in range(0, self.WMAX, 3):  # records that encode values >= p
            masked[i] = masked[i][:15] + b"\xEE"
        masked[1] = b"\xFF" * 16
        self.masked = masked
        tuples = [(rng.randrange(self.p).to_bytes(16, "little"), rng.randrange(self.p).to_bytes(16, "little"))
                  for _ in range(self.WMAX)]
        self.tup = np.frombuffer(b"".join(a + b for a, b in tuples), np.uint8).reshape(-1, 32)
        self.tup.setflags(write=False)
        self.share = {uz: np.frombuffer(O.convert_to_secret_share(spdz, masked, str(self.key), tuples, uz),
                                        np.uint8).reshape(-1, 32) for uz in (False, True)}

    def texts(self, sizes):
        wo = offsets_of(sizes)
        return [data_text(self.masked[int(wo[o]):int(wo[o + 1])]) for o in range(len(sizes))]

    def single(self, text: bytes, w0: int, W: int, uz: bool):
        """amph_convert_share_json on one object alone (host) -> (rows or None, bad)."""
        import amphora_amd as A
        lib = A._lib.lib
        out, bad = np.zeros((W, 32), np.uint8), C.c_int64(-7)
        tup = np.ascontiguousarray(self.tup[w0:w0 + W])
        st = lib.amph_convert_share_json(self.ctx._h, text, len(text), W, tup.ctypes.data,
                                         self.key.to_bytes(16, "little"), int(uz), out.ctypes.data, C.byref(bad), 0,
                                         None)
        assert st in (OK, E_PARAM) and (st == OK) == (bad.value == -1), (st, lib.amph_last_error())
        return (out if st == OK else None), bad.value


@pytest.fixture(scope="module", params=["big", "small"])
def conv(request):
    return ConvCase(request.param)


def dense(texts):
    """The dense concatenation and its byte offsets."""
    toff = np.concatenate([[0], np.cumsum([len(t) for t in texts])]).astype(np.uint64)[:len(texts)]
    return b"".join(texts), toff


def conv_run(c, sizes, texts, uz, mode, toff=None, blob=None):
    """One call -> (list of per-object share rows, bad[K] with -1 clean, status, message)."""
    wo = offsets_of(sizes)
    T = int(wo[-1])
    if blob is None:
        blob, toff = dense(texts)
    if mode == "host_batch":
        outs, bad, st = c.ctx.convert_share_json_batch(
            texts, [np.ascontiguousarray(c.tup[int(wo[o]):int(wo[o + 1])]) for o in range(len(sizes))], c.key, uz,
            status=True)
        return outs, list(bad), st[0], st[1]
    if mode == "host_packed":
        out, bad, st = c.ctx.convert_share_json_packed(blob, wo, toff, np.ascontiguousarray(c.tup[:T]), c.key, uz,
                                                       status=True)
    else:
        import torch
        tx = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
        out, bad, st = c.ctx.convert_share_json_packed(tx, _dev(wo), _dev(toff), _dev(c.tup[:T]), c.key, uz,
                                                       status=True)
        out, bad = _host(out), _host(bad)
    return [out[int(wo[o]):int(wo[o + 1])] for o in range(len(sizes))], list(bad), st[0], st[1]


def conv_check(c, sizes, texts, res, uz, bad=None):
    """Against the oracle and against the single call on each object alone;
    bad = {object: offset}: those objects' rows are unspecified."""
    bad = bad or {}
    outs, got_bad = res[0], res[1]
    wo = offsets_of(sizes)
    assert [int(x) for x in got_bad] == [bad.get(o, -1) for o in range(len(sizes))]
    for o, W in enumerate(sizes):
        w0 = int(wo[o])
        rows, sbad = c.single(texts[o], w0, W, uz)
        assert sbad == bad.get(o, -1), o
        if o in bad:
            continue
        assert outs[o].shape == (W, 32)
        assert np.array_equal(outs[o], c.share[uz][w0:w0 + W]), o
        assert np.array_equal(outs[o], rows), o


# ---- 1. parity per object -------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("uz", [False, True])
def test_convert_parity_per_object(conv, mode, uz):
    texts = conv.texts(CONV_SIZES)
    assert [len(t) for t in texts] == [data_chars(W) for W in CONV_SIZES]
    _, toff = dense(texts)
    assert len({int(t) & 15 for t in toff}) >= 6 and any(int(t) & 1 for t in toff)  # (2.) dense: odd alignments
    res = conv_run(conv, CONV_SIZES, texts, uz, mode)
    assert res[2] == OK, res[3]
    conv_check(conv, CONV_SIZES, texts, res, uz)


# ---- 2. alignment ---------------------------------------------------------------
@pytest.mark.parametrize("mode", ["host_packed", "device_packed"])
def test_every_text_alignment(conv, mode):
    """Three objects, each placed at every residue of 16 as `a` sweeps; the
    bytes between and around the texts are record openers (never consumed)."""
    sizes = [129, 17, 128]
    texts = conv.texts(sizes)
    wo = offsets_of(sizes)
    seen = [set(), set(), set()]
    for a in range(16):
        toff, at = [], a
        for o, gap in enumerate((5, 11, 3)):
            toff.append(at)
            seen[o].add(at & 15)
            at += len(texts[o]) + gap
        blob = bytearray((b',{"value":"' * (at // 11 + 2))[:at + 16])
        for o in range(3):
            blob[toff[o]:toff[o] + len(texts[o])] = texts[o]
        res = conv_run(conv, sizes, texts, False, mode, np.array(toff, np.uint64), bytes(blob))
        assert res[2] == OK and res[1] == [-1, -1, -1], (a, res[3])
        for o in range(3):
            assert np.array_equal(res[0][o], conv.share[False][int(wo[o]):int(wo[o + 1])]), (a, o)
    assert all(len(s) == 16 for s in seen)


# ---- 3. rejections (convert) -----------------------------------------------------
def _alter(ch: int) -> int:
    return {ord(","): ord("]"), ord("]"): ord(",")}.get(ch, ch ^ 0x20)


def _with(texts, faults):
    """texts with {object: [(offset, new byte or None = _alter)]} applied."""
    out = list(texts)
    for o, fs in faults.items():
        t = bytearray(out[o])
        for off, new in fs:
            t[off] = _alter(t[off]) if new is None else new
            assert t[off] != texts[o][off]
        out[o] = bytes(t)
    return out


@pytest.mark.parametrize("mode", MODES)
def test_faults_keep_to_their_objects(conv, mode):
    # objects 1 (1 word), 3 (127), 5 (129: its second tile), 7 (257: two faults, the smaller wins in
    # either text order) are refused; 2, 4, 8 and the empty 0, 6 in between stay clean
    faults = {1: [(1 + 12, ord("*"))], 3: [(1 + 37 * 126 + 36, None)], 5: [(1 + 37 * 128 + 3, None)],
              7: [(1 + 37 * 200 + 35, ord("!")), (1 + 37 * 9 + 20, ord("!"))]}
    texts = _with(conv.texts(CONV_SIZES), faults)
    want = {o: min(off for off, _ in fs) for o, fs in faults.items()}
    assert want[3] == 37 * 127 and want[7] == 1 + 37 * 9 + 20
    res = conv_run(conv, CONV_SIZES, texts, False, mode)
    conv_check(conv, CONV_SIZES, texts, res, False, bad=want)
    if mode != "device_packed":
        assert res[2] == E_PARAM
        assert "object 1" in res[3] and "offset 13" in res[3] and "record 0" in res[3] and "4 of 9" in res[3], res[3]


@pytest.mark.parametrize("mode", MODES)
def test_framing_is_each_objects_own(conv, mode):
    """Dense concatenation: object o + 1's '[' follows object o's ']' directly."""
    clean = conv.texts(CONV_SIZES)
    cases = [
        {4: [(0, None)]},                         # an object's '[' altered
        {4: [(37 * 128, ord("X"))]},              # its final ']' altered
        {3: [(37 * 127, ord(","))]},              # a ',' where object 3's final ']' belongs
        {0: [(0, ord("{"))], 6: [(1, ord("["))]},  # "[]" of an empty object, either byte: 0 and 1
        {0: [(1, ord(","))], 6: [(0, ord("]"))]},
        {8: [(0, ord(","))], 7: [(37 * 257, ord(","))]},  # "...},[{..." read as one array
    ]
    for faults in cases:
        texts = _with(clean, faults)
        want = {o: fs[0][0] for o, fs in faults.items()}
        res = conv_run(conv, CONV_SIZES, texts, False, mode)
        conv_check(conv, CONV_SIZES, texts, res, False, bad=want)


def _rejections(W):
    """(offset, replacement byte) of every single fault of tests/test_upload_wire.py's
    list, restated: on a record of the object's first tile and on its last record."""
    out = []
    for rec in (5, W - 1):
        base = 1 + 37 * rec
        for ch in (0, 15, 16, 21):  # a byte outside the alphabet
            out.append((base + 10 + ch, b"*-\x80 "[ch % 4]))
        out.append((base + 10 + 21, ord("=")))
        out.append((base + 10 + 22, ord("A")))
        out.append((base + 10 + 23, ord("A")))
        for k in list(range(10)) + [34, 35, 36]:  # the 13 frame bytes
            out.append((base + k, None))
    out.append((0, None))
    return out


def test_every_single_fault_on_a_middle_object(conv):
    import torch
    sizes = [128, 129, 2]  # the middle object ends in a tile of one record, at an odd alignment
    clean = conv.texts(sizes)
    wo, T = offsets_of(sizes), sum(sizes)
    dwo, tup = _dev(wo), _dev(conv.tup[:T])
    cases = _rejections(129)
    assert (37 * 129, None) in cases
    for off, new in cases:
        texts = _with(clean, {1: [(off, new)]})
        blob, toff = dense(texts)
        tx = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
        out, bad = conv.ctx.convert_share_json_packed(tx, dwo, _dev(toff), tup, conv.key, False)
        assert list(_host(bad)) == [-1, off, -1], (off, new)
        out = _host(out)
        for o in (0, 2):
            assert np.array_equal(out[int(wo[o]):int(wo[o + 1])], conv.share[False][int(wo[o]):int(wo[o + 1])])
    assert conv.single(_with(clean, {1: [cases[0]]})[1], 128, 129, False)[1] == cases[0][0]


# ================================================================ client side
class MaskCase:
    """n parties' Input Mask ODOs per object (its own synth_odos call), one
    secret per mask word, the oracle's masked words and texts, object by
    object.  faults = {object: failing word}."""

    def __init__(self, kind, n, sizes, faults=None, seed=5000):
        self.kind, self.n, self.sizes = kind, n, list(sizes)
        p, r, rinv = FIELDS[kind]
        self.ctx = _ctx(kind)
        Fd = coracle.Field(p, r, rinv, threads=4)
        util = O.ClientSecretShareUtil(p, r, rinv)
        rng = random.Random(seed + n)
        faults = faults or {}
        self.texts, self.secrets, self.expect, self.ff = [], [], [], []
        for o, W in enumerate(sizes):
            if W == 0:
                e = np.zeros((0, 16), np.uint8)
                odos = [tuple(e for _ in range(5)) for _ in range(n)]
                sec, exp = [], b"[]"
            else:
                odos, _ = Fd.synth_odos(seed=seed + 17 * o + n, n=n, W=W, noncanon_permille=100,
                                        fault_index=faults.get(o, -1))
                sec = [rng.randrange(p) for _ in range(W)]
                exp = None
                if o not in faults:
                    ref = [O.OutputDeliveryObject(*[np.ascontiguousarray(f).tobytes() for f in od]) for od in odos]
                    exp = data_text(O.create_secret_masked_inputs(util, sec, ref))
            self.texts.append([[base64.b64encode(np.ascontiguousarray(f).tobytes()) for f in od] for od in odos])
            self.secrets.append(np.frombuffer(b"".join(s.to_bytes(16, "little") for s in sec), np.uint8)
                                .reshape(-1, 16))
            self.expect.append(exp)
            self.ff.append(faults.get(o, -1))
        self.woff = offsets_of(sizes)

    def slots(self):
        """Dense 16-aligned input slots: (text_offsets, field buffers per party)."""
        toff, at = [], 0
        for W in self.sizes:
            toff.append(at)
            at += -(-nchars_of(W) // 16) * 16
        nchars = max(at, 16)
        bufs = []
        for j in range(self.n):
            fs = []
            for k in range(5):
                b = np.full(nchars, ord("!"), np.uint8)
                for o in range(len(self.sizes)):
                    t = self.texts[o][j][k]
                    b[toff[o]:toff[o] + len(t)] = np.frombuffer(t, np.uint8)
                fs.append(b)
            bufs.append(tuple(fs))
        return np.array(toff, np.uint64), bufs

    def single(self, o):
        """amph_mask_input_json on object o alone (host): (text or None, ff, bad)."""
        try:
            return self.ctx.mask_input_json(self.texts[o], self.sizes[o], self.secrets[o])
        except ValueError:  # a bad character
            return None, -1, -2


@functools.lru_cache(maxsize=None)
def mask_case(kind, n):
    return MaskCase(kind, n, MASK_SIZES)


def mask_run(c, mode):
    """-> (list of per-object texts, ff[K], bad[K], status)."""
    K = len(c.sizes)
    if mode == "host_batch":
        texts, ff, bad, st = c.ctx.mask_input_json_batch(c.texts, c.sizes, c.secrets, status=True)
        return texts, list(ff), list(bad), st[0]
    toff, bufs = c.slots()
    sec = np.ascontiguousarray(np.concatenate(c.secrets))
    if mode == "host_packed":
        out, oo, ff, bad, st = c.ctx.mask_input_json_packed(bufs, c.woff, toff, sec, status=True)
    else:
        out, oo, ff, bad, st = c.ctx.mask_input_json_packed([tuple(_dev(f) for f in p) for p in bufs], _dev(c.woff),
                                                            _dev(toff), _dev(sec), status=True)
        out, oo, ff, bad = _host(out), _host(oo), _host(ff), _host(bad)
    assert all(int(x) % 16 == 0 for x in oo)
    texts = [out[int(oo[o]):int(oo[o]) + data_chars(c.sizes[o])].tobytes() for o in range(K)]
    return texts, list(ff), list(bad), st[0]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind,n", [("big", 1), ("big", 2), ("big", 3), ("small", 1), ("small", 2), ("small", 3)])
def test_mask_parity_per_object(kind, n, mode):
    c = mask_case(kind, n)
    texts, ff, bad, st = mask_run(c, mode)
    assert st == OK and ff == [-1] * len(c.sizes) and bad == [-1] * len(c.sizes)
    for o, W in enumerate(c.sizes):
        assert len(c.expect[o]) == data_chars(W)
        assert texts[o] == c.expect[o], o
        if mode == "host_packed":  # (the single call's result does not depend on the mode compared with)
            assert c.single(o) == (c.expect[o], -1, -1), o


# ---- 4. rejections (mask) ----------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_mask_verdicts_are_per_object(mode):
    c = MaskCase("big", 2, MASK_SIZES, faults={4: 192}, seed=5100)
    t = bytearray(c.texts[2][1][3])  # object 2 (191 words), party 1's wShares
    t[700] = ord("*")
    c.texts[2][1][3] = bytes(t)
    texts, ff, bad, st = mask_run(c, mode)
    want_bad = (5 * 1 + 3) * nchars_of(191) + 700
    assert bad == [want_bad if o == 2 else -1 for o in range(7)]
    assert [ff[o] for o in range(7) if o != 2] == [192 if o == 4 else -1 for o in range(7) if o != 2]
    if mode != "device_packed":
        assert st == E_PARAM and ff[2] == -1
    for o in (0, 1, 3, 5, 6):
        assert texts[o] == c.expect[o], o
    assert c.single(2)[2] == -2 and c.single(4)[1] == 192  # the single calls' verdicts


# ---- 5. extents ------------------------------------------------------------------
def _outside(g, spans):
    """The payload bytes of output g outside [a, b) spans kept their pattern."""
    keep = np.ones(g.n, bool)
    for a, b in spans:
        keep[a:b] = False
    before, after = g.before[g.lo:g.lo + g.n], g.after[g.lo:g.lo + g.n]
    d = np.nonzero((before != after) & keep)[0]
    assert d.size == 0, "%s: byte %d outside every object's output changed" % (g.name, int(d[0]))


@pytest.mark.parametrize("fill", ["zeros", "hostile"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_convert_extents(conv, device, fill):
    import amphora_amd as A
    texts = conv.texts(CONV_SIZES)
    blob, toff = dense(texts)
    wo, K, T = offsets_of(CONV_SIZES), len(CONV_SIZES), sum(CONV_SIZES)
    main = X.Arena(device)
    g_x = main.add("texts", X.JSONTXT, data=blob, offset=5, fill=fill)
    g_w = main.add("woff", X.OFFS, data=wo, fill=fill)
    g_t = main.add("toff", X.OFFS, data=toff, fill=fill)
    g_u = main.add("tuples", X.WORD, data=np.ascontiguousarray(conv.tup[:T]), fill=fill)
    g_o = main.add("shares", X.WORD, n=32 * T)
    g_b = main.add("bad", X.VERDICT, n=8 * K)
    main.commit()
    st = A._lib.lib.amph_convert_share_json_packed(conv.ctx._h, g_x.ptr, len(blob), g_w.ptr, g_t.ptr, K, g_u.ptr,
                                                   conv.key.to_bytes(16, "little"), 0, g_o.ptr, g_b.ptr,
                                                   F_DEVICE if device else 0, None)
    if device:
        import torch
        torch.cuda.synchronize()
    main.fetch()
    for g in main.items:
        (g.check_untouched if g in (g_o, g_b) else g.check_unchanged)()  # rows [0, T), entries [0, K) only
    assert st == OK
    assert list(np.frombuffer(g_b.payload(), np.int64)) == [NF if device else -1] * K
    assert g_o.payload() == conv.share[False][:T].tobytes()


@pytest.mark.parametrize("fill", ["zeros", "hostile"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_mask_extents(device, fill):
    """Output slots with gaps of 16-64 bytes: nothing outside each object's own
    characters is written -- the slot's tail after its ']', the gaps, the bands."""
    import amphora_amd as A
    c = mask_case("big", 2)
    K, T = len(c.sizes), sum(c.sizes)
    toff, bufs = c.slots()
    ooff, at = [], 32
    for o, W in enumerate(c.sizes):
        ooff.append(at)
        at += -(-data_chars(W) // 16) * 16 + 16 * ((3 * o + 1) % 5)
    cap = at
    main = X.Arena(device)
    g_in = {(j, k): main.add("t%d%d" % (j, k), X.B64, data=bufs[j][k], fill=fill) for j in range(2) for k in range(5)}
    g_w = main.add("woff", X.OFFS, data=c.woff, fill=fill)
    g_t = main.add("toff", X.OFFS, data=toff, fill=fill)
    g_oo = main.add("ooff", X.OFFS, data=np.array(ooff, np.uint64), fill=fill)
    g_s = main.add("secrets", X.WORD, data=np.concatenate(c.secrets), fill=fill)
    g_x = main.add("out_text", X.WORD, n=cap)
    g_ff = main.add("ff", X.VERDICT, n=8 * K)
    g_bad = main.add("bad", X.VERDICT, n=8 * K)
    main.commit()
    arr = (A._lib._AmphOdoB64 * 2)()
    for j in range(2):
        arr[j] = A._lib._AmphOdoB64(*[g_in[(j, k)].ptr for k in range(5)], len(bufs[0][0]))
    st = A._lib.lib.amph_mask_input_json_packed(c.ctx._h, arr, 2, g_w.ptr, g_t.ptr, K, g_s.ptr, g_x.ptr, cap,
                                                g_oo.ptr, g_ff.ptr, g_bad.ptr, F_DEVICE if device else 0, None)
    if device:
        import torch
        torch.cuda.synchronize()
    main.fetch()
    outs = (g_x, g_ff, g_bad)
    for g in main.items:
        (g.check_untouched if g in outs else g.check_unchanged)()
    assert st == OK, A._lib.lib.amph_last_error()
    none = NF if device else -1
    assert list(np.frombuffer(g_ff.payload(), np.int64)) == [none] * K
    assert list(np.frombuffer(g_bad.payload(), np.int64)) == [none] * K
    got = g_x.payload()
    for o, W in enumerate(c.sizes):
        assert got[ooff[o]:ooff[o] + data_chars(W)] == c.expect[o], o
    _outside(g_x, [(ooff[o], ooff[o] + data_chars(W)) for o, W in enumerate(c.sizes)])


# ---- 6. broken device tables -------------------------------------------------------
@pytest.mark.parametrize("table", ["decreasing", "above-T"])
def test_broken_device_tables_stay_inside_the_write_bounds(conv, table):
    """AMPH_F_DEVICE leaves the tables to the caller; whatever they hold, no
    share row past T = word_offsets[K] and no verdict entry outside [0, K) is
    written.  All text_offsets are 0 over a buffer that holds a full T-word
    text, so every read a clamped tile can make lies inside the buffers: a tile
    of the clamped range [w0, w1) within [0, T] reads text bytes up to
    37 (w1 - w0) + 1 <= 37 T + 1 and tuple rows below T.  Only the write bounds
    are asserted, nothing about values."""
    import amphora_amd as A
    import torch
    T, K = 300, 4
    wo = np.array({"decreasing": [0, 200, 100, 260, T], "above-T": [0, 100, 5000, 290, T]}[table], np.uint64)
    text = data_text(conv.masked[:T])
    main = X.Arena(True)
    g_x = main.add("texts", X.JSONTXT, data=text, offset=0, fill="zeros")
    g_w = main.add("woff", X.OFFS, data=wo, fill="zeros")
    g_t = main.add("toff", X.OFFS, data=np.zeros(K, np.uint64), fill="zeros")
    g_u = main.add("tuples", X.WORD, data=np.ascontiguousarray(conv.tup[:T]), fill="zeros")
    g_o = main.add("shares", X.WORD, n=32 * T)
    g_b = main.add("bad", X.VERDICT, n=8 * K)
    main.commit()
    st = A._lib.lib.amph_convert_share_json_packed(conv.ctx._h, g_x.ptr, len(text), g_w.ptr, g_t.ptr, K, g_u.ptr,
                                                   conv.key.to_bytes(16, "little"), 0, g_o.ptr, g_b.ptr, F_DEVICE,
                                                   None)
    torch.cuda.synchronize()
    main.fetch()
    assert st == OK
    for g in main.items:
        (g.check_untouched if g in (g_o, g_b) else g.check_unchanged)()


# ---- 7. copies and launches -----------------------------------------------------------
def conv_run_ctx(ctx, c, sizes):
    """A clean host batch call on ctx -> (copies, launches) it took."""
    wo = offsets_of(sizes)
    c0, l0 = ctx.upload_batch_copies(), ctx.stats()["kernel_launches"]
    outs, bad = ctx.convert_share_json_batch(
        c.texts(sizes), [np.ascontiguousarray(c.tup[int(wo[o]):int(wo[o + 1])]) for o in range(len(sizes))], c.key,
        False)
    assert list(bad) == [-1] * len(sizes)
    assert b"".join(o.tobytes() for o in outs) == c.share[False][:sum(sizes)].tobytes()
    return ctx.upload_batch_copies() - c0, ctx.stats()["kernel_launches"] - l0


def test_convert_copies_and_launches_do_not_grow_with_k():
    import amphora_amd as A
    kind = "big"
    p, r, rinv = FIELDS[kind]
    ctx = A.Context(p, r, rinv)
    c = ConvCase(kind)
    res = conv_run_ctx(ctx, c, CONV_SIZES)  # 645 words: the small-call arena
    assert res == (0, 1)
    T = 25600
    assert T * (37 + 32 + 32) > (2 << 20)  # above the default AMPH_SMALL_BYTES: the staged path
    rng = random.Random(99)
    spdz = O.MpSpdzIntegrationUtils(p, r, rinv)
    masked = [rng.randrange(1 << 128).to_bytes(16, "little") for _ in range(T)]
    tuples = [(rng.randrange(p).to_bytes(16, "little"), rng.randrange(p).to_bytes(16, "little")) for _ in range(T)]
    want = O.convert_to_secret_share(spdz, masked, str(c.key), tuples, False)
    tup = np.frombuffer(b"".join(a + b for a, b in tuples), np.uint8).reshape(-1, 32)
    deltas = []
    for K in (2, 64):
        W = T // K
        texts = [data_text(masked[o * W:(o + 1) * W]) for o in range(K)]
        c0, l0 = ctx.upload_batch_copies(), ctx.stats()["kernel_launches"]
        outs, bad = ctx.convert_share_json_batch(texts, [tup[o * W:(o + 1) * W] for o in range(K)], c.key, False)
        deltas.append((ctx.upload_batch_copies() - c0, ctx.stats()["kernel_launches"] - l0))
        assert list(bad) == [-1] * K and b"".join(o.tobytes() for o in outs) == want
    assert deltas == [(2, 1), (2, 1)]


def test_mask_copies_and_launches_do_not_grow_with_k():
    import amphora_amd as A
    p, r, rinv = FIELDS["big"]
    ctx = A.Context(p, r, rinv)
    c = mask_case("big", 1)
    c0, l0 = ctx.upload_batch_copies(), ctx.stats()["kernel_launches"]
    texts, ff, bad = ctx.mask_input_json_batch(c.texts, c.sizes, c.secrets)  # 962 words x 1 party: the arena
    assert texts == c.expect and (ctx.upload_batch_copies() - c0, ctx.stats()["kernel_launches"] - l0) == (0, 1)
    T, n = 12800, 2
    assert T * 10 * 64 // 3 > (2 << 20)  # the field texts alone are above AMPH_SMALL_BYTES
    Fd = coracle.Field(p, r, rinv, threads=4)
    odos, _ = Fd.synth_odos(seed=808, n=n, W=T, noncanon_permille=50)
    sec = Fd.synth_words(seed=809, count=T, mont=False)
    masked, eff = Fd.mask_input(sec, odos)  # (the C restatement: see the module docstring)
    assert eff == -1
    deltas = []
    for K in (2, 64):
        W = T // K
        objs = [[[base64.b64encode(np.ascontiguousarray(f[o * W:(o + 1) * W]).tobytes()) for f in od] for od in odos]
                for o in range(K)]
        c0, l0 = ctx.upload_batch_copies(), ctx.stats()["kernel_launches"]
        texts, ff, bad = ctx.mask_input_json_batch(objs, [W] * K, [sec[o * W:(o + 1) * W] for o in range(K)])
        deltas.append((ctx.upload_batch_copies() - c0, ctx.stats()["kernel_launches"] - l0))
        assert list(ff) == [-1] * K and list(bad) == [-1] * K
        assert texts == [data_text(masked[o * W:(o + 1) * W]) for o in range(K)]
    assert deltas == [(2, 1), (2, 1)]


# ---- 8. device round trip -------------------------------------------------------------
@pytest.mark.parametrize("kind", ["big", "small"])
def test_device_round_trip_client_to_parties(kind):
    """mask_input_json_packed's out_text and out_text_offsets go straight in as
    convert_share_json_packed's texts / text_offsets, for each of 2 parties."""
    c = mask_case(kind, 2)
    p = FIELDS[kind][0]
    spdz = O.MpSpdzIntegrationUtils(*FIELDS[kind])
    toff, bufs = c.slots()
    sec = np.ascontiguousarray(np.concatenate(c.secrets))
    dwo = _dev(c.woff)
    out_text, oo, ff, bad = c.ctx.mask_input_json_packed([tuple(_dev(f) for f in q) for q in bufs], dwo, _dev(toff),
                                                         _dev(sec))
    masked = [w for o in range(len(c.sizes)) for w in
              [base64.b64decode(d["value"]) for d in json.loads(c.expect[o])]]  # the oracle's masked words
    T = len(masked)
    rng = random.Random(31)
    for party in range(2):
        key = rng.randrange(1, p)
        tuples = [(rng.randrange(p).to_bytes(16, "little"), rng.randrange(p).to_bytes(16, "little"))
                  for _ in range(T)]
        tup = np.frombuffer(b"".join(a + b for a, b in tuples), np.uint8).reshape(T, 32)
        share, cbad = c.ctx.convert_share_json_packed(out_text, dwo, oo, _dev(tup), key, party != 0)
        assert list(_host(cbad)) == [-1] * len(c.sizes)
        assert _host(share).tobytes() == O.convert_to_secret_share(spdz, masked, str(key), tuples, party != 0)
    assert list(_host(ff)) == [-1] * len(c.sizes) and list(_host(bad)) == [-1] * len(c.sizes)


# ---- 9. mirrors -------------------------------------------------------------------------
def test_service_mirror_gives_the_single_functions_outcomes(conv):
    from amphora_amd.service import SecretShareUtil
    util = SecretShareUtil(conv.ctx)
    tags = [{"key": "k", "value": "v", "valueType": "STRING"}]

    def body(w0, W, pretty=False, values=None, sid="80fbba1b-3da8-4b1e-8a2c-cebd65229fad"):
        vals = values if values is not None else [base64.b64encode(w).decode() for w in conv.masked[w0:w0 + W]]
        obj = {"secretId": sid, "data": [{"value": v} for v in vals], "tags": tags}
        return json.dumps(obj, indent=2) if pretty else json.dumps(obj, separators=(",", ":"))

    refused = body(300, 129).replace('"value":"', '"value":"*', 1).replace('=="}', '="}', 1)
    uploads = [  # (body, first word, masks' words)
        (body(0, 129), 0, 129),                 # compact
        (body(129, 40, pretty=True), 129, 40),  # pretty-printed
        (body(169, 20), 169, 21),               # wrong count
        (refused, 300, 129),                    # a refused byte in a compact body
        (body(0, 0), 0, 0),                     # empty
        (body(429, 130).encode(), 429, 130),    # compact, as bytes
        (body(200, 3, sid=None), 200, 3),       # compact, and the remainder's own verdict
    ]
    masks = [np.ascontiguousarray(conv.tup[w0:w0 + W]) for _, w0, W in uploads]
    for uz in (False, True):
        singles = []
        for (b, _, _), m in zip(uploads, masks):
            try:
                singles.append(util.convert_masked_input_json(b, str(conv.key), m, uz))
            except Exception as e:  # noqa: BLE001 -- compared below
                singles.append(e)
        before = conv.ctx.stats()["kernel_launches"]
        got = util.convert_masked_inputs_json([b for b, _, _ in uploads], str(conv.key), masks, uz)
        assert len(got) == len(uploads)
        for i, (g, s) in enumerate(zip(got, singles)):
            if isinstance(s, Exception):
                assert type(g) is type(s) and str(g) == str(s), (i, g, s)
            else:
                assert (g.secret_id, g.data, g.tags) == (s.secret_id, s.data, s.tags), i
        assert [isinstance(g, Exception) for g in got] == [False, False, True, True, False, False, True]
        for i in (0, 1, 5):  # and the values themselves come from the oracle
            _, w0, W = uploads[i]
            assert got[i].data == conv.share[uz][w0:w0 + W].tobytes()
        assert got[4].data == b""
        assert conv.ctx.stats()["kernel_launches"] - before >= 1


def test_client_mirror_equals_the_records_form():
    import amphora_amd as A
    from amphora_amd import client, wire
    c = MaskCase("big", 2, [3, 192, 1, 193, 5, 40], faults={3: 100}, seed=5200)
    ctx = c.ctx
    util = client.SecretShareUtil(ctx)
    sids = [uuid.UUID(int=7000 + o) for o in range(6)]

    def bodies(o, texts=None):
        out = []
        for j in range(c.n):
            d = {name: (texts or c.texts[o])[j][k].decode("latin-1")
                 for k, name in enumerate(("secretShares", "rShares", "vShares", "wShares", "uShares"))}
            out.append(json.dumps(d, separators=(",", ":")))
        return out

    bad_texts = [list(q) for q in c.texts[4]]
    bad_texts[1][2] = bad_texts[1][2][:10] + b"!" + bad_texts[1][2][11:]  # object 4: a bad character
    lists = [bodies(o, bad_texts if o == 4 else None) for o in range(6)]
    secrets = [A.Secret.of([("k", "v")] if o == 1 else [], client.unpack(c.secrets[o]), secret_id=sids[o])
               for o in range(6)]
    secrets[5] = A.Secret.of([], client.unpack(c.secrets[5])[:7], secret_id=sids[5])  # fewer secrets: irregular
    want = client.create_masked_inputs_from_bodies(util, secrets, lists)
    got = client.create_masked_input_bodies(util, secrets, lists)
    assert len(got) == len(want) == 6
    for i, (g, w) in enumerate(zip(got, want)):
        if isinstance(w, Exception):
            assert type(g) is type(w) and str(g) == str(w), (i, g, w)
        else:
            assert g == w, i
    assert isinstance(got[3], A.IntegrityVerificationException) and isinstance(got[4], A.AmphoraClientException)
    assert [isinstance(g, str) for g in got] == [True, True, True, False, False, True]
    for o in (0, 1, 2):  # the oracle's text inside the body
        assert json.dumps(json.loads(got[o])["data"], separators=(",", ":")).encode() == c.expect[o]
    assert got[0] == wire.records_to_masked_input_json(
        sids[0], np.frombuffer(b"".join(d["value"].encode() for d in json.loads(c.expect[0])), np.uint8)
        .reshape(-1, 24), [])
