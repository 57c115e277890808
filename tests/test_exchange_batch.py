"""Many requests' Beaver exchange texts per call, on the GPU
(include/amphora_exchange_batch.h: amph_exchange_encode_packed / _batch,
amph_exchange_decode_packed / _batch; kernels k_xencs_* / k_xdecs_*).

Every object is checked against what the project already trusts: Jackson's
compact text of its signed Python integers (tests/extent_cases.jackson), those
integers themselves, and the single calls amph_exchange_encode /
amph_exchange_decode on that object alone.  256 pairs are one encode tile and
8,192 characters one decode span: the size lists sit on both edges of each,
with empty objects first, in the middle and last.  Each test asserts its
coverage predicates on its own inputs before the call."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import amphora_oracle as O
from oracle import coracle
from tests import exchange_cases as EC
from tests import extent_cases as X
from tests import field_cases as FC
from tests.test_exchange_batch_cpu import BROKEN_DEVICE_TABLES

pytestmark = pytest.mark.gpu

P, R, RINV = O.TEST_PRIME, O.TEST_R, O.TEST_RINV
NF = 0x7F7F7F7F7F7F7F7F
OK, E_LEN, E_PARAM = 0, 2, 3
F_DEVICE, F_ACCUMULATE, F_HOST_IO = 1, 2, 4
SPAN = 8192
MODES = ["host_packed", "host_batch", "device_packed"]
PAIRS = [0, 1, 2, 255, 256, 257, 0, 513, 1024, 0]


@functools.lru_cache(maxsize=None)
def _ctx():
    import amphora_amd as A
    return A.Context(P, R, RINV)


def _L():
    import amphora_amd
    return amphora_amd._lib


def _dev(x):
    import torch
    x = np.array(x, copy=True)
    return torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).cuda()


def _host(v):
    import torch
    torch.cuda.synchronize()
    return v.cpu().numpy()


def max_chars(p):
    return 92 * p + 2


def slot_chars(p):
    return -(-max_chars(p) // SPAN) * SPAN


def offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)


def diffs(vals):
    """(magnitude, negative flag) values -> mag (P, 2, 16), neg (P, 2), the signed integers, the decoder's signs."""
    mag = FC.arr([v for v, _ in vals]).reshape(-1, 2, 16)
    neg = np.array([g for _, g in vals], np.uint8).reshape(-1, 2)
    signed = [-v if g else v for v, g in vals]
    dneg = np.array([1 if g and v else 0 for v, g in vals], np.uint8).reshape(-1, 2)  # no "-0" in a text
    return mag, neg, signed, dneg


def text_of(signed):
    return X.jackson(list(zip(signed[0::2], signed[1::2])))


# ---- 1. object sizes against the 256-pair tile ----------------------------------------
@functools.lru_cache(maxsize=None)
def size_case():
    """2 sum(PAIRS) values: every decimal length 1..39 in turn, every 41st a
    special -- 10^k, 2^k, 2^128 - 1, a signed zero."""
    T = sum(PAIRS)
    special = [10 ** k for k in (0, 1, 8, 9, 16, 31, 32, 38)] + [2 ** k for k in (1, 32, 63, 64, 96, 127)] + \
        [FC.MASK128, 0]
    vals = []
    for i in range(2 * T):
        if i % 41 == 40:
            v = special[(i // 41) % len(special)]
            vals.append((v, 1 if (i // 41) % 2 == 0 or v == 0 else 0))
            continue
        n = 1 + i % 39
        v = i % 10 if n == 1 else 10 ** (n - 1) + (i * 7919) % (10 ** (n - 1))
        vals.append((v, 1 if i % 3 == 0 else 0))
    mag, neg, signed, dneg = diffs(vals)
    poff = offsets(PAIRS)
    texts = [text_of(signed[2 * int(poff[o]):2 * int(poff[o + 1])]) for o in range(len(PAIRS))]
    seen = {len(str(v)) for v, _ in vals}
    assert seen == set(range(1, 40)) and (0, 1) in vals
    assert any(v == FC.MASK128 for v, _ in vals) and any(v == 10 ** 38 for v, _ in vals)
    assert texts[0] == b"[]" and texts[6] == b"[]" and texts[9] == b"[]"
    for a in (mag, neg, dneg):
        a.setflags(write=False)
    return mag, neg, dneg, poff, texts


def slots(counts, gap):
    toff, at = [], 0
    for p in counts:
        toff.append(at)
        at += slot_chars(p) + gap
    return np.array(toff, np.uint64), at


def encode(mode, mag, neg, poff, gap=0):
    """-> (texts[o], out_lens, whole buffer or None, its fill, text_offsets)."""
    ctx = _ctx()
    counts = [int(b - a) for a, b in zip(poff, poff[1:])]
    K = len(counts)
    if mode == "host_batch":
        texts = ctx.exchange_encode_batch([mag[int(poff[o]):int(poff[o + 1])] for o in range(K)],
                                          [neg[int(poff[o]):int(poff[o + 1])] for o in range(K)])
        return texts, np.array([len(t) for t in texts]), None, None, None
    toff, cap = slots(counts, gap)
    fill = X.band_pattern(11, cap + 64)  # 64 characters behind the last slot as well
    if mode == "host_packed":
        out, to, lens = ctx.exchange_encode_packed(mag, neg, poff, toff, out=fill.copy())
        lens = np.asarray(lens)
    else:
        out, to, lens = ctx.exchange_encode_packed(_dev(mag), _dev(neg), _dev(poff), _dev(toff), out=_dev(fill))
        out, to, lens = _host(out), _host(to), _host(lens)
    assert [int(x) for x in to] == [int(x) for x in toff]
    texts = [out[int(toff[o]):int(toff[o]) + int(lens[o])].tobytes() for o in range(K)]
    return texts, lens, out, fill, toff


def check_gaps(out, fill, toff, lens):
    keep = np.ones(fill.size, bool)
    for o in range(len(toff)):
        keep[int(toff[o]):int(toff[o]) + int(lens[o])] = False
    d = np.nonzero((out != fill) & keep)[0]
    assert d.size == 0, "character %d outside every text changed" % int(d[0])


@pytest.mark.parametrize("mode,gap", [(m, g) for m in MODES for g in (0, SPAN) if m != "host_batch" or not g])
def test_encode_sizes_against_the_tile(mode, gap):
    mag, neg, _, poff, want = size_case()
    assert PAIRS[0] == PAIRS[6] == PAIRS[-1] == 0 and {255, 256, 257, 513, 1024} <= set(PAIRS)
    texts, lens, out, fill, toff = encode(mode, mag, neg, poff, gap)
    for o in range(len(PAIRS)):
        assert texts[o] == want[o], "object %d (%d pairs)" % (o, PAIRS[o])
        assert int(lens[o]) == len(want[o]), o
    if out is not None:
        check_gaps(out, fill, toff, lens)


def test_encode_equals_the_single_call_per_object():
    mag, neg, _, poff, want = size_case()
    ctx = _ctx()
    for o in (1, 3, 5, 7):
        a, b = int(poff[o]), int(poff[o + 1])
        assert ctx.exchange_encode(mag[a:b], neg[a:b]) == want[o], o


@pytest.mark.parametrize("mode", MODES)
def test_decode_sizes_against_the_tile(mode):
    mag, _, dneg, poff, texts = size_case()
    got_mag, got_neg, bad, _ = decode(mode, texts, PAIRS)
    assert [int(x) for x in bad] == [-1] * len(PAIRS)
    assert np.array_equal(got_mag, mag) and np.array_equal(got_neg, dneg)


# ---- 2. texts against the 8 KiB span --------------------------------------------------
def sized_text(length, seed):
    """The values of a compact object of exactly `length` characters, by the choice of digit lengths."""
    npairs = (length - 1) // 40
    budget = length - 1 - 12 * npairs  # digits and signs of the 2 npairs values
    nsign = (2 * npairs + 4) // 5      # every fifth value negative
    digits = budget - nsign
    base, extra = divmod(digits, 2 * npairs)
    assert 1 <= base and base + 1 <= 39
    vals = []
    for i in range(2 * npairs):
        n = base + (1 if i < extra else 0)
        v = (seed + i) % 9 + 1 if n == 1 else 10 ** (n - 1) + ((seed + i) * 7919) % (10 ** (n - 1))
        vals.append((v, 1 if i % 5 == 0 else 0))
    return vals


HOSTILE = b'1234567890:,{"a":7,"b":8},{"a":'


@functools.lru_cache(maxsize=None)
def span_case():
    """Objects: 8191, 8192, 8193 and 16384 characters; 720 one-digit pairs
    (more than 256 colons per span); a compact one, a whitespace-and-"b","a"
    one, a compact one; an empty one.  -> (texts, pair counts, mag, dneg)."""
    texts, counts, allvals = [], [], []
    for k, n in enumerate((8191, 8192, 8193, 16384)):
        vals = sized_text(n, 100 * k)
        texts.append(text_of(diffs(vals)[2]))
        assert len(texts[-1]) == n, (len(texts[-1]), n)
        counts.append(len(vals) // 2)
        allvals += vals
    vals = [((i * 7) % 10, 1 if i % 4 == 1 else 0) for i in range(1440)]
    t = text_of(diffs(vals)[2])
    first = t[:SPAN].count(b":")
    assert len(vals) // 2 >= 700 and 256 < first < 1280 and len(t) > SPAN, first  # past the dense head, below kMaxStarts
    texts.append(t)
    counts.append(720)
    allvals += vals
    for kind in ("compact", "spaced", "compact"):
        vals = sized_text(9000, 7)[:400]
        signed = diffs(vals)[2]
        if kind == "spaced":
            body = " ,\n".join('{ "b" :%d ,\t"a": %d }' % (b, a) for a, b in zip(signed[0::2], signed[1::2]))
            t = ("[ " + body + " ]\r\n").encode()
            assert b" " in t and t.index(b'"b"') < t.index(b'"a"') and len(t) > SPAN
        else:
            t = text_of(signed)
        texts.append(t)
        counts.append(200)
        allvals += vals
    texts.append(b"[]")
    counts.append(0)
    mag, _, _, dneg = diffs(allvals)
    mag.setflags(write=False)
    dneg.setflags(write=False)
    return tuple(texts), tuple(counts), mag, dneg


def pack_texts(texts, fill, gap=0):
    """-> (buffer, text_offsets, text_lens): every text at its span-aligned slot of a buffer otherwise `fill`."""
    toff, at = [], 0
    for t in texts:
        toff.append(at)
        at += max(SPAN, -(-len(t) // SPAN) * SPAN) + gap
    buf = np.frombuffer((fill * (at // len(fill) + 1))[:at], np.uint8).copy()
    for t, a in zip(texts, toff):
        buf[a:a + len(t)] = np.frombuffer(t, np.uint8)
    return buf, np.array(toff, np.uint64), np.array([len(t) for t in texts], np.uint64)


def decode(mode, texts, counts, fill=b" ", gap=0, lens=None, accumulate_into=None):
    """-> (mag (T, 2, 16), neg (T, 2), bad_index as host ints: -1 = clean,
    (status, message) of a host call or None), the packed modes through slots
    whose rest and gaps hold `fill`."""
    ctx = _ctx()
    poff = offsets(counts)
    if mode == "host_batch":
        res, bad, st = ctx.exchange_decode_batch(list(texts), list(counts), status=True)
        mag = np.concatenate([m for m, _ in res]) if res else np.zeros((0, 2, 16), np.uint8)
        neg = np.concatenate([g for _, g in res]) if res else np.zeros((0, 2), np.uint8)
        return mag, neg, bad, st
    buf, toff, tl = pack_texts(texts, fill, gap)
    if lens is not None:
        tl = np.array(lens, np.uint64)
    if mode == "host_packed":
        mag, neg, bad, st = ctx.exchange_decode_packed(buf, poff, toff, tl, status=True)
        return mag, neg, bad, st
    mag, neg, bad = ctx.exchange_decode_packed(_dev(buf), poff, _dev(toff), _dev(tl),  # (a host pair table: it sizes
                                               bad_index=accumulate_into,             # the outputs, and goes to the
                                               accumulate=accumulate_into is not None)  # device with the call)
    bad = _host(bad)
    return _host(mag), _host(neg), np.where(bad == NF, -1, bad), None


@pytest.mark.parametrize("mode", MODES)
def test_decode_texts_against_the_span(mode):
    texts, counts, mag, dneg = span_case()
    assert [len(t) for t in texts[:4]] == [8191, 8192, 8193, 16384]
    got = [decode(mode, texts, counts, fill=f, gap=g) for f, g in ((b" ", 0), (HOSTILE, 0), (HOSTILE, SPAN))]
    for m, g, bad, _ in got:
        assert [int(x) for x in bad] == [-1] * len(texts)
        assert np.array_equal(m, mag) and np.array_equal(g, dneg)


def test_decode_equals_the_single_call_per_object():
    texts, counts, mag, dneg = span_case()
    ctx, poff = _ctx(), offsets(counts)
    for o in (0, 4, 6):
        m, g = ctx.exchange_decode(texts[o], counts[o])
        a, b = int(poff[o]), int(poff[o + 1])
        assert np.array_equal(m, mag[a:b]) and np.array_equal(g, dneg[a:b]), o


# ---- 3. faults, one object at a time ----------------------------------------------------
@functools.lru_cache(maxsize=None)
def fault_base():
    """Four clean objects: a span and a half, a small one, one span and one character, a small one."""
    vals = [sized_text(12000, 3), sized_text(500, 5), sized_text(SPAN + 1, 9), sized_text(300, 11)]
    texts = [text_of(diffs(v)[2]) for v in vals]
    counts = [len(v) // 2 for v in vals]
    assert len(texts[0]) > SPAN + 100 and len(texts[2]) == SPAN + 1
    mag, _, _, dneg = diffs([x for v in vals for x in v])
    return texts, counts, mag, dneg


def _poke(t, at, byte=b"x"):
    return t[:at] + byte + t[at + 1:]


def fault_cases():
    """name -> (object, its text, its pair count, its text_lens entry or None)."""
    texts, counts, _, _ = fault_base()
    big, small, over = texts[0], texts[1], texts[2]
    two128 = small.replace(b'{"a":', b'{"a":%d,"b":1},{"a":' % (2 ** 128), 1)
    return {
        "bad-first-byte": (1, _poke(small, 0), counts[1], None),
        "bad-last-byte": (1, _poke(small, len(small) - 1), counts[1], None),
        "bad-before-span-border": (0, _poke(big, SPAN - 1), counts[0], None),
        "bad-after-span-border": (0, _poke(big, SPAN), counts[0], None),
        # without its ']' the text fills its slot exactly: the next slot's '[' follows it directly
        "missing-bracket-next-slot-opens": (2, over[:-1], counts[2], None),
        "one-pair-too-few": (1, small, counts[1] + 1, None),
        "one-pair-too-many": (1, small, counts[1] - 1, None),
        "magnitude-2^128": (1, two128, counts[1] + 1, None),
        "empty-text": (1, small, counts[1], 0),
        "empty-array-one-pair": (1, b"[]", 1, None),
        "no-pairs-one-present": (1, b'[{"a":1,"b":2}]', 0, None),
    }


def single_verdict(text, npairs):
    """(status, bad_index) of amph_exchange_decode on one text alone; they are
    those of the header's rule (tests/exchange_cases.first_bad)."""
    L, ctx = _L(), _ctx()
    a = np.frombuffer(text, np.uint8) if text else np.zeros(1, np.uint8)
    mag, neg = np.zeros((npairs + 1, 32), np.uint8), np.zeros((npairs + 1, 2), np.uint8)
    bad = C.c_int64(-1)
    st = L.lib.amph_exchange_decode(ctx._h, a.ctypes.data, len(text), npairs, mag.ctypes.data, neg.ctypes.data,
                                    C.byref(bad), 0, None)
    rule = EC.first_bad(text, npairs)
    assert (st, bad.value) == ({"ok": OK, "param": E_PARAM, "len": E_LEN}[rule.kind], rule.bad), (st, bad.value, rule)
    return st, bad.value


@pytest.mark.parametrize("name", sorted(fault_cases()))
@pytest.mark.parametrize("mode", MODES)
def test_one_faulty_object_moves_only_its_own_verdict(mode, name):
    texts, counts, mag, dneg = fault_base()
    obj, text, npairs, tlen = fault_cases()[name]
    ftexts, fcounts = list(texts), list(counts)
    ftexts[obj], fcounts[obj] = text, npairs
    lens = None
    if tlen is not None:
        lens = [len(t) for t in ftexts]
        lens[obj] = tlen
        if mode == "host_batch":
            ftexts[obj] = text[:tlen]
    if name == "missing-bracket-next-slot-opens":  # the text fills its slot: the next slot's '[' follows it directly
        assert len(text) == SPAN and not text.endswith(b"]") and texts[obj + 1].startswith(b"[")
        buf, toff, tl = pack_texts(ftexts, HOSTILE)
        assert int(toff[obj + 1]) == int(toff[obj]) + int(tl[obj])
        assert bytes(buf[int(toff[obj + 1]) - 1:int(toff[obj + 1]) + 1]) == b"}["
    want_st, want_bad = single_verdict(text if tlen is None else text[:tlen], npairs)
    assert want_st in (E_PARAM, E_LEN) and want_bad >= 0, (want_st, want_bad)
    fill = HOSTILE
    got_mag, got_neg, bad, status = decode(mode, ftexts, fcounts, fill=fill, lens=lens)
    assert [int(x) for x in bad] == [want_bad if o == obj else -1 for o in range(4)], (bad, want_bad)
    # every other object's rows: bit-identical to the clean run
    po, fo = offsets(counts), offsets(fcounts)
    for o in range(4):
        if o != obj:
            assert np.array_equal(got_mag[int(fo[o]):int(fo[o + 1])], mag[int(po[o]):int(po[o + 1])]), o
            assert np.array_equal(got_neg[int(fo[o]):int(fo[o + 1])], dneg[int(po[o]):int(po[o + 1])]), o
    if status is not None:  # host modes: the single call's status, naming the object
        st, msg = status
        assert st == want_st and ("object %d:" % obj) in msg and "1 of 4 texts refused" in msg, (st, msg)
        if want_st == E_PARAM:
            assert ("offset %d " % want_bad) in msg, msg


def test_host_status_prefers_a_refused_text_over_a_count_mismatch():
    texts, counts, _, _ = fault_base()
    ftexts, fcounts = list(texts), list(counts)
    fcounts[1] += 1                                   # a count mismatch first ...
    ftexts[3] = _poke(texts[3], 5)                    # ... a refused text later
    _, _, bad, (st, msg) = decode("host_packed", ftexts, fcounts)
    assert st == E_PARAM and "object 3:" in msg and "2 of 4 texts refused" in msg, (st, msg)
    assert int(bad[1]) == len(texts[1]) and int(bad[3]) >= 0 and int(bad[0]) == int(bad[2]) == -1
    ftexts[3] = texts[3]
    _, _, _, (st, msg) = decode("host_batch", ftexts, fcounts)
    assert st == E_LEN and "object 1:" in msg and "exactly %d FactorPairs" % fcounts[1] in msg, (st, msg)


# ---- 4. capacity --------------------------------------------------------------------------
def test_gather_encode_with_one_capacity_short():
    mag, neg, _, poff, want = size_case()
    ctx = _ctx()
    objs = [1, 3, 4, 0]
    caps = [len(want[o]) for o in objs]
    caps[1] -= 1
    texts, lens, (st, msg) = ctx.exchange_encode_batch([mag[int(poff[o]):int(poff[o + 1])] for o in objs],
                                                       [neg[int(poff[o]):int(poff[o + 1])] for o in objs],
                                                       out_caps=caps, status=True)
    assert st == E_LEN and "object 1:" in msg, (st, msg)
    assert [int(x) for x in lens] == [len(want[o]) for o in objs]
    assert texts == [want[1], None, want[4], want[0]]


def test_gather_encode_leaves_a_short_buffer_untouched():
    L, ctx = _L(), _ctx()
    mag, neg, _, poff, want = size_case()
    m, g = np.ascontiguousarray(mag[1:3]), np.ascontiguousarray(neg[1:3])
    out = np.full(256, 0x55, np.uint8)
    lens = np.zeros(1, np.uint64)
    st = L.lib.amph_exchange_encode_batch(ctx._h, (C.c_void_p * 1)(m.ctypes.data), (C.c_void_p * 1)(g.ctypes.data),
                                          (C.c_size_t * 1)(2), 1, (C.c_void_p * 1)(out.ctypes.data),
                                          (C.c_size_t * 1)(len(want[2]) - 1), lens.ctypes.data, 0)
    assert st == E_LEN and int(lens[0]) == len(want[2]) and (out == 0x55).all()


def test_host_packed_slot_below_max_chars_launches_nothing():
    ctx = _ctx()
    mag, neg = np.zeros((90, 2, 16), np.uint8), np.zeros((90, 2), np.uint8)
    before = ctx.stats()["kernel_launches"]
    with pytest.raises(_L().AmphoraNativeError, match="out_cap"):
        ctx.exchange_encode_packed(mag, neg, [0, 90], [0], out=np.zeros(max_chars(90) - 1, np.uint8))
    assert ctx.stats()["kernel_launches"] == before


# ---- 5. launch count, copies, flags ---------------------------------------------------------
def test_launch_count_does_not_depend_on_the_object_count():
    """amph_ctx_stats().kernel_launches counts a call's launch sequences (one
    per LaunchCfg the ABI hands a launcher), not its kernels: every call here
    must add exactly one whatever K is, which a loop of launcher calls over
    the objects would break.  That the sequence itself is fixed (four kernels
    for an encode, six for a decode, the scan always in its two-launch form)
    is the launchers' construction, launch_exchange_*_seg; this counter does
    not see it."""
    import amphora_amd as A
    mag, neg, _, poff, texts = size_case()
    ctx = _ctx()

    def delta(fn):
        a = ctx.stats()["kernel_launches"]
        fn()
        return ctx.stats()["kernel_launches"] - a

    def calls(K):
        po = poff[:K + 1]
        T = int(po[-1])
        m, g, tx, cnt = mag[:T], neg[:T], list(texts[:K]), PAIRS[:K]
        buf, toff, tl = pack_texts(tx, b" ")
        return [
            lambda: ctx.exchange_encode_packed(m, g, po),
            lambda: ctx.exchange_encode_batch([m[int(po[o]):int(po[o + 1])] for o in range(K)],
                                              [g[int(po[o]):int(po[o + 1])] for o in range(K)]),
            lambda: ctx.exchange_decode_packed(buf, po, toff, tl),
            lambda: ctx.exchange_decode_batch(tx, cnt),
            lambda: ctx.exchange_encode_packed(_dev(m), _dev(g), _dev(po), _dev(slots(cnt, 0)[0]),
                                               out=_dev(np.zeros(slots(cnt, 0)[1], np.uint8))),
            lambda: ctx.exchange_decode_packed(_dev(buf), _dev(po), _dev(toff), _dev(tl), npairs_total=T),
        ]
    one, ten = [delta(f) for f in calls(1)], [delta(f) for f in calls(10)]
    assert one == ten == [1] * 6, (one, ten)
    # the copies: none on the arena path, two per staged call
    c0 = ctx.exchange_batch_copies()
    for f in calls(10)[:4]:
        f()
    assert ctx.exchange_batch_copies() == c0
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("AMPH_SMALL_BYTES", "0")
        staged = A.Context(P, R, RINV)
    po = poff
    buf, toff, tl = pack_texts(list(texts), b" ")
    out, to, lens = staged.exchange_encode_packed(mag, neg, po)
    assert staged.exchange_batch_copies() == 2
    assert [out[int(to[o]):int(to[o]) + int(lens[o])].tobytes() for o in range(len(PAIRS))] == list(texts)
    m2, g2, bad = staged.exchange_decode_packed(buf, po, toff, tl)
    assert staged.exchange_batch_copies() == 4 and list(bad) == [-1] * len(PAIRS) and np.array_equal(m2, mag)
    staged.exchange_encode_batch([mag[:1]], [neg[:1]])
    staged.exchange_decode_batch([texts[1]], [1])
    assert staged.exchange_batch_copies() == 8


def test_device_decode_accumulates_on_request():
    import torch
    texts, counts, _, _ = fault_base()
    ftexts = list(texts)
    ftexts[1] = _poke(texts[1], 9)
    want = single_verdict(ftexts[1], counts[1])[1]
    prior = torch.tensor([NF, 3, 5, NF], dtype=torch.int64, device="cuda")
    _, _, bad, _ = decode("device_packed", ftexts, counts, accumulate_into=prior)
    assert [int(x) for x in bad] == [-1, min(3, want), 5, -1]
    _, _, bad, _ = decode("device_packed", ftexts, counts)  # without the flag: reset first
    assert [int(x) for x in bad] == [-1, want, -1, -1]


def test_host_io_is_refused_and_no_objects_are_accepted():
    L, ctx = _L(), _ctx()
    z = np.zeros(64, np.uint64)
    p = z.ctypes.data
    for fl in (F_HOST_IO, F_HOST_IO | F_DEVICE):
        assert L.lib.amph_exchange_encode_packed(ctx._h, p, p, 0, p, p, 1, p, 64, p, fl, None) == E_PARAM
        assert L.lib.amph_exchange_decode_packed(ctx._h, p, 64, p, p, p, 1, 0, p, p,
                                                 C.cast(C.c_void_p(p), C.POINTER(C.c_int64)), fl, None) == E_PARAM
    before = ctx.stats()["kernel_launches"]
    for fl in (0, F_DEVICE):
        assert L.lib.amph_exchange_encode_packed(ctx._h, None, None, 0, None, None, 0, None, 0, None, fl, None) == OK
        assert L.lib.amph_exchange_decode_packed(ctx._h, None, 0, None, None, None, 0, 0, None, None, None, fl,
                                                 None) == OK
    assert ctx.stats()["kernel_launches"] == before


# ---- 6. broken device tables ----------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(BROKEN_DEVICE_TABLES))
def test_broken_device_tables_stay_inside_the_arrays(name):
    """The device calls take the tables as they are (the contract is the
    caller's): the calls return, every guard band is intact and only the K
    words of out_lens / bad_index are written.  tests/test_exchange_batch_cpu.py
    has passed the same tables through the geometry header's bounds check."""
    import torch
    L, ctx = _L(), _ctx()
    npairs, cap, poff, toff, lens = BROKEN_DEVICE_TABLES[name]
    K = len(toff)
    rng = np.random.default_rng(5)
    text = np.frombuffer((HOSTILE * (cap // len(HOSTILE) + 1))[:cap], np.uint8)
    arena = X.Arena(True)
    g = {
        "mag": arena.add("mag", X.WORD, data=rng.integers(0, 256, 32 * npairs, dtype=np.uint8)),
        "neg": arena.add("neg", X.SIGN, data=rng.integers(0, 2, 2 * npairs, dtype=np.uint8)),
        "poff": arena.add("poff", X.OFFS, data=np.array(poff, np.uint64)),
        "toff": arena.add("toff", X.OFFS, data=np.array(toff, np.uint64)),
        "tlen": arena.add("tlen", X.OFFS, data=np.array(lens, np.uint64)),
        "text": arena.add("text", X.XCHG, data=text, offset=0),
        "out": arena.add("out", X.XCHG, n=cap, offset=0),
        "lens": arena.add("lens", X.OFFS, n=8 * K),
        "omag": arena.add("omag", X.WORD, n=32 * npairs),
        "oneg": arena.add("oneg", X.SIGN, n=2 * npairs),
        "bad": arena.add("bad", X.VERDICT, n=8 * K),
    }
    arena.commit()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    st = L.lib.amph_exchange_encode_packed(ctx._h, g["mag"].ptr, g["neg"].ptr, npairs, g["poff"].ptr, g["toff"].ptr,
                                           K, g["out"].ptr, cap, g["lens"].ptr, F_DEVICE, s)
    assert st == OK, L.lib.amph_last_error()
    st = L.lib.amph_exchange_decode_packed(ctx._h, g["text"].ptr, cap, g["poff"].ptr, g["toff"].ptr, g["tlen"].ptr,
                                           K, npairs, g["omag"].ptr, g["oneg"].ptr, X.i64(g["bad"].ptr), F_DEVICE, s)
    assert st == OK, L.lib.amph_last_error()
    torch.cuda.synchronize()
    arena.fetch()
    for k in ("mag", "neg", "poff", "toff", "tlen", "text"):
        g[k].check_unchanged()
    for k in ("out", "lens", "omag", "oneg", "bad"):
        g[k].check_untouched()


# ---- 7. the device round trip, no host synchronisation ---------------------------------------
def test_three_parties_round_trip_on_one_stream():
    """odo_pre on the concatenation of K = 6 requests (one empty), every
    party's encode, every party's decode of its partners' buffers as they are,
    open_post -- all on one stream with no host read in between: the inputs
    arrive behind a time-based gate (tests/stream_cases.py), so the device
    holds zeros while every call is made, and the stream has not passed the
    gate when the last call returns.  The K ODOs equal the oracle's per
    request; a verdict planted on one partner object leaves the other
    requests' w and u equal to the oracle's."""
    import time
    import torch
    from tests import stream_cases as S
    ctx = _ctx()
    F = coracle.test_field(threads=8)
    n, words = 3, [3, 0, 130, 1, 64, 257]
    K, W = len(words), sum(words)
    woff = [int(x) for x in offsets(words)]
    pcounts = [2 * w for w in words]  # two pairs per word
    assert 0 in pcounts and any(p % 256 for p in pcounts) and max(pcounts) > 256
    shares = [F.synth_words(seed=100 + j, count=2 * W).reshape(W, 32) for j in range(n)]
    masks = [F.synth_words(seed=200 + j, count=4 * W).reshape(2 * W, 32) for j in range(n)]
    triples = [F.synth_words(seed=300 + j, count=12 * W).reshape(2 * W, 96) for j in range(n)]
    # the oracle, request by request
    want = []  # want[j][o] = (y, r, v, w, u)
    for j in range(n):
        want.append([])
    for o in range(K):
        a, b = woff[o], woff[o + 1]
        pre = [F.odo_pre(shares[j][a:b], 32, masks[j][2 * a:2 * b], triples[j][2 * a:2 * b]) if b > a else None
               for j in range(n)]
        for j in range(n):
            if b == a:
                want[j].append(None)
                continue
            order = [j] + [k for k in range(n) if k != j]
            opened = F.recombine_diffs([pre[k][3] for k in order], [pre[k][4] for k in order])
            w, u = F.odo_post(opened, triples[j][2 * a:2 * b], j == 0)
            want[j].append((pre[j][0], pre[j][1], pre[j][2], w, u))
    poff = offsets(pcounts)
    toff, cap = slots(pcounts, 0)
    hit = 2
    host = {"poff": poff.view(np.int64), "toff": toff.view(np.int64)}
    for j in range(n):
        host.update({"shares%d" % j: shares[j], "masks%d" % j: masks[j], "triples%d" % j: triples[j]})
    pinned = {k: torch.from_numpy(np.ascontiguousarray(v)).pin_memory() for k, v in host.items()}

    took = []  # (host ms, step) of the last chain: which call waited, if one did

    def step(what, fn):
        t0 = time.perf_counter()
        res = fn()
        took.append((round(1e3 * (time.perf_counter() - t0), 3), what))
        return res

    def chain(d):
        """Every call of the exchange on the current stream, device tensors in and out, nothing read on the host."""
        del took[:]
        pre = [step("odo_pre %d" % j, lambda j=j: ctx.odo_pre(d["shares%d" % j], 32, d["masks%d" % j],
                                                              d["triples%d" % j])) for j in range(n)]
        bufs = step("output buffers", lambda: [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(n)])
        enc = [step("encode %d" % j, lambda j=j: ctx.exchange_encode_packed(pre[j][3], pre[j][4], d["poff"], d["toff"],
                                                                            out=bufs[j])) for j in range(n)]

        def party(j):
            mags, negs, bads = [pre[j][3]], [pre[j][4]], []
            for q in range(n):
                if q != j:
                    m, g, bad = step("decode %d<-%d" % (j, q), lambda q=q: ctx.exchange_decode_packed(
                        enc[q][0], d["poff"], enc[q][1], enc[q][2], npairs_total=int(poff[-1])))
                    mags.append(m)
                    negs.append(g)
                    bads.append(bad)
            return step("open_post %d" % j, lambda: ctx.open_post(mags, negs, d["triples%d" % j], j == 0)), bads
        outs = [party(j) for j in range(n)]
        # party 1's text of request 2 damaged in place, party 0 opens again
        step("damage", lambda: enc[1][0][int(toff[hit]) + 7:int(toff[hit]) + 8].fill_(ord("x")))
        return pre, outs, party(0)

    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):  # ungated first: code objects, the scratch and torch's blocks
        chain({k: v.cuda(non_blocking=True) for k, v in pinned.items()})
    stream.synchronize()
    gate = S.Gate()
    dz = {k: torch.zeros(v.shape, dtype=v.dtype, device="cuda") for k, v in pinned.items()}
    torch.cuda.synchronize()
    before = torch.cuda.Event()
    with torch.cuda.stream(stream):  # the inputs arrive behind the gate: the device holds zeros while the calls are made
        gate.enqueue()
        for k, v in pinned.items():
            dz[k].copy_(v, non_blocking=True)
        before.record()
        t0 = time.perf_counter()
        pre, outs, again = chain(dz)
        host_ms = 1e3 * (time.perf_counter() - t0)
        reached = before.query()
    stream.synchronize()
    print("round trip: %d steps enqueued in %.3f ms on the host, gate %.3f ms" % (len(took), host_ms, gate.measured_ms))
    assert not reached, "the stream had passed the gate when the last call returned: the calls took %.3f ms on the " \
        "host, the gate is %.3f ms; the slowest: %r" % (host_ms, gate.measured_ms, sorted(took, reverse=True)[:4])

    def same(got, j, skip=None):
        (w, u), _ = got
        w, u = _host(w), _host(u)
        for o in range(K):
            if want[j][o] is not None and o != skip:
                a, b = woff[o], woff[o + 1]
                assert np.array_equal(w[a:b], want[j][o][3]) and np.array_equal(u[a:b], want[j][o][4]), (j, o)
    for j in range(n):
        assert all((_host(b) == NF).all() for b in outs[j][1]), j
        same(outs[j], j)
        y, r, v = (_host(x) for x in pre[j][:3])
        for o in range(K):
            if want[j][o] is not None:
                a, b = woff[o], woff[o + 1]
                assert all(np.array_equal(g[a:b], e) for g, e in zip((y, r, v), want[j][o][:3])), (j, o)
    bads = [_host(b) for b in again[1]]
    a, b = woff[hit], woff[hit + 1]
    t = ctx.exchange_encode(*F.odo_pre(shares[1][a:b], 32, masks[1][2 * a:2 * b], triples[1][2 * a:2 * b])[3:5])
    want_bad = single_verdict(_poke(t, 7), pcounts[hit])[1]
    assert want_bad >= 0
    assert [int(x) for x in bads[0]] == [NF if o != hit else want_bad for o in range(K)]  # partner 1 is party 0's first
    assert (bads[1] == NF).all()
    same(again, 0, skip=hit)


# ---- 8. the stream contract -------------------------------------------------------------------
def stream_plans():
    """The two device packed calls as extent plans (tests/stream_cases.py)."""
    mag, neg, dneg, poff, texts = size_case()
    K = len(PAIRS)
    toff, cap = slots(PAIRS, 0)
    lens = [len(t) for t in texts]

    def check_enc(whole):
        out = whole["out"]
        for o in range(K):
            assert out[int(toff[o]):int(toff[o]) + lens[o]] == texts[o], o

    enc = X.Plan("exchange_encode_packed K=%d" % K,
                 [X.Arr("mag", X.WORD, data=mag), X.Arr("neg", X.SIGN, data=neg), X.Arr("poff", X.OFFS, data=poff),
                  X.Arr("toff", X.OFFS, data=toff)],
                 [X.Arr("out", X.XCHG, n=cap, offset=0),
                  X.Arr("lens", X.OFFS, n=8 * K, expect=b"".join(X.le8(x) for x in lens))],
                 lambda L, h, p, fl, s: L.amph_exchange_encode_packed(h, p["mag"], p["neg"], int(poff[-1]), p["poff"],
                                                                      p["toff"], K, p["out"], cap, p["lens"], fl, s),
                 check=check_enc)
    buf, dtoff, dlens = pack_texts(list(texts), HOSTILE)
    dec = X.Plan("exchange_decode_packed K=%d" % K,
                 [X.Arr("text", X.XCHG, data=buf, offset=0), X.Arr("poff", X.OFFS, data=poff),
                  X.Arr("toff", X.OFFS, data=dtoff), X.Arr("tlen", X.OFFS, data=dlens)],
                 [X.Arr("mag", X.WORD, n=mag.size, expect=X.raw(mag)), X.Arr("neg", X.SIGN, n=dneg.size,
                                                                             expect=X.raw(dneg)),
                  X.Arr("bad", X.VERDICT, verdict=[-1] * K)],
                 lambda L, h, p, fl, s: L.amph_exchange_decode_packed(h, p["text"], buf.size, p["poff"], p["toff"],
                                                                      p["tlen"], K, int(poff[-1]), p["mag"], p["neg"],
                                                                      X.i64(p["bad"]), fl, s))
    return [enc, dec]


def test_device_calls_keep_to_their_stream():
    """Inputs arrive behind a gate on the stream: the call returns before the
    gate opens (no wait), and the results equal the reference (order)."""
    import torch
    from tests import stream_cases as S
    L, ctx = _L(), _ctx()
    gate, stream = S.Gate(), torch.cuda.Stream()
    for plan in stream_plans():
        sp = C.c_void_p(stream.cuda_stream)

        def invoke(ins, outs, plan=plan):
            p = {k: g.ptr for k, g in list(ins.items()) + list(outs.items())}
            return plan.call(L.lib, ctx._h, p, F_DEVICE, sp)
        S.run_plan_deferred(plan, invoke, stream, None, fill="zeros")  # ungated: the first-use allocations
        d = S.run_plan_deferred(plan, invoke, stream, gate, no_wait=True)
        assert d.reached is False


@pytest.mark.parametrize("device", [False, True])
def test_packed_calls_respect_their_arrays(device):
    """P1-P4 of tests/extent_cases.py for both packed calls: guard bands around
    every array, inputs unchanged, results independent of the bytes around them."""
    import torch
    L, ctx = _L(), _ctx()
    for plan in stream_plans():
        def invoke(ins, outs, plan=plan):
            p = {k: g.ptr for k, g in list(ins.items()) + list(outs.items())}
            s = C.c_void_p(torch.cuda.current_stream().cuda_stream) if device else None
            return plan.call(L.lib, ctx._h, p, F_DEVICE if device else 0, s)
        X.run_plan(plan, device, invoke, sync=torch.cuda.synchronize if device else None)


# ---- 9. the Python mirrors ------------------------------------------------------------------
def test_wire_mirrors_equal_the_single_functions_body_by_body():
    import uuid
    from amphora_amd import wire
    ctx = _ctx()
    mag, neg, dneg, poff, texts = size_case()
    objs = [1, 0, 3, 5, 9]
    ops = [uuid.UUID(int=4100 + o) for o in objs]
    ms = [mag[int(poff[o]):int(poff[o + 1])] for o in objs]
    gs = [neg[int(poff[o]):int(poff[o + 1])] for o in objs]
    bodies = wire.exchange_bodies_to_json(ctx, ops, 2, ms, gs)
    assert bodies == [wire.exchange_to_json(ctx, op, 2, m, g) for op, m, g in zip(ops, ms, gs)]
    assert wire.exchange_bodies_to_json(ctx, [], 0, [], []) == [] and wire.exchange_bodies_from_json(ctx, [], []) == []
    broken = list(bodies)
    broken[2] = bodies[2].replace(b'"a":', b'"a":x', 1)            # a malformed number
    broken[3] = bodies[3].replace(b'"interimValues"', b'"values"')  # no interimValues member
    counts = [PAIRS[o] for o in objs]
    counts[0] += 1                                                  # a count mismatch
    got = wire.exchange_bodies_from_json(ctx, broken, counts)
    for k in range(len(objs)):
        try:
            want = wire.exchange_from_json(ctx, broken[k], counts[k])
        except Exception as e:  # noqa: BLE001 -- the single function's outcome for this body
            want = e
        if isinstance(want, Exception):
            assert k in (0, 2, 3) and type(got[k]) is type(want) and str(got[k]) == str(want), (k, got[k], want)
        else:
            assert got[k][:2] == want[:2] == (ops[k], 2), k
            assert np.array_equal(got[k][2], want[2]) and np.array_equal(got[k][3], want[3]), k


class Cluster:
    """n loopback parties over the fake dealer, with K secrets uploaded."""

    def __init__(self, n, sizes, seed):
        import random
        from concurrent.futures import ThreadPoolExecutor
        import amphora_amd as A
        from amphora_amd.loopback import AmphoraParty, ExchangeHub, LoopbackAmphoraClient
        from tests.loopback_dealer import FakeCastor
        rng = random.Random(seed)
        keys = [rng.randrange(P) for _ in range(n)]
        self.castor = FakeCastor(P, R, RINV, keys, seed)
        self.hub = ExchangeHub(n, timeout_s=20)
        self.parties = [AmphoraParty(j, P, R, RINV, keys[j], self.castor, self.hub, exchange_format="json")
                        for j in range(n)]
        self.client = LoopbackAmphoraClient(self.parties, P, R, RINV)
        self.sids = [self.client.create_secret(A.Secret.of([("n", str(o))], [rng.randrange(P) for _ in range(W)]))
                     for o, W in enumerate(sizes)]
        self.pool = ThreadPoolExecutor(max_workers=n)

    def all(self, fn):
        return [f.result() for f in [self.pool.submit(fn, p) for p in self.parties]]

    def close(self):
        self.pool.shutdown()
        self.client.close()


def test_service_mirror_with_json_bodies_three_parties():
    """compute_output_delivery_objects with exchange_format="json", n = 3,
    K = 5: bit for bit the per-request loop; the launches of the whole call do
    not grow with K; one request's malformed partner body turns that request
    alone into the single function's exception."""
    import uuid
    import amphora_amd as A
    from amphora_amd import service, wire
    sizes = [1, 130, 5, 64, 3]
    K = len(sizes)
    c = Cluster(3, sizes, seed=47)
    try:
        rids = [uuid.UUID(int=888000 + o) for o in range(K)]

        def launches(fn):
            before = [p.ctx.stats()["kernel_launches"] for p in c.parties]
            res = c.all(fn)
            return res, [p.ctx.stats()["kernel_launches"] - b for p, b in zip(c.parties, before)]
        batch, all_k = launches(lambda p: p.odo_service.compute_output_delivery_objects(
            [p.secrets[s] for s in c.sids], rids))
        _, two = launches(lambda p: p.odo_service.compute_output_delivery_objects(
            [p.secrets[s] for s in c.sids[:2]], rids[:2]))
        assert all_k == two, (all_k, two)
        singles = [c.all(lambda p, o=o: p.odo_service.compute_output_delivery_object(p.secrets[c.sids[o]], rids[o]))
                   for o in range(K)]
        for j in range(3):
            for o in range(K):
                assert isinstance(batch[j][o], A.OutputDeliveryObject), (j, o, batch[j][o])
                assert list(batch[j][o].fields()) == list(singles[o][j].fields()), (j, o)
        # party 0 alone (the hub holds the partners' bodies of every operation): request 3's first partner body damaged
        p0 = c.parties[0]
        svc = p0.odo_service
        exchange = svc._exchange
        bad_op = service.name_uuid_from_bytes(("%s_%d" % (rids[3], 2 * sizes[3])).encode())

        def damaging_exchange(body):
            partners = [bytes(b) for b in exchange(body)]
            if wire.exchange_header(bytes(body))[0] == bad_op:
                partners[0] = partners[0].replace(b'"b":', b'"b":!', 1)
            return partners
        svc._exchange = damaging_exchange
        try:
            got = svc.compute_output_delivery_objects([p0.secrets[s] for s in c.sids], rids)
            with pytest.raises(A.AmphoraServiceException) as single:
                svc.compute_output_delivery_object(p0.secrets[c.sids[3]], rids[3])
        finally:
            svc._exchange = exchange
        assert type(got[3]) is A.AmphoraServiceException and str(got[3]) == str(single.value)
        assert str(got[3]) == "Failed to open values for operation #%s" % bad_op
        assert str(got[3].__cause__) == str(single.value.__cause__)
        for o in range(K):
            if o != 3:
                assert list(got[o].fields()) == list(batch[0][o].fields()), o
    finally:
        c.close()
