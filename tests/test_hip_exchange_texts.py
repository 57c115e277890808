"""The exchange-text catalogue (tests/exchange_cases.py) through every call that
reads a Beaver exchange text, on the GPU: the five names of EC.MATRIX, each
`_dev` sibling through its base name, host and device mode where the header has
both.  Every expectation is the catalogue's -- `first_bad` for the verdict,
`parse_pairs` for the values, the C oracle on those values for a session's
fields -- and none comes from the library.  The cases run as the objects of one
call (or, for the calls that take one text, without a host wait between them),
so each test takes seconds.

For a refused text only what the headers define is asserted: the status, the
verdict, the message, a free slot or poisoned fields; that object's outputs are
unspecified.  Everything else is exact.
"""
import base64
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import amphora_oracle as O
from tests import exchange_cases as EC
from tests import field_cases as FC
from tests.test_exchange_batch import E_LEN, E_PARAM, HOSTILE, NF, OK, decode, offsets

pytestmark = pytest.mark.gpu

P, R, RINV = O.TEST_PRIME, O.TEST_R, O.TEST_RINV
FORMS = ["single", "packed", "batch", "party", "parties"]
STATUS = {"ok": OK, "param": E_PARAM, "len": E_LEN}
EVERYTHING = "FULL+EDGE+NUMBERS+PAIRS+ACCEPTED"
MALFORMED = "Malformed FactorPair JSON at offset %d"
COUNT = "interimValues must hold exactly %d FactorPairs"


@functools.lru_cache(maxsize=None)
def _ctx():
    import amphora_amd as A
    return A.Context(P, R, RINV)


def _L():
    import amphora_amd
    return amphora_amd._lib


@functools.lru_cache(maxsize=None)
def _F():
    from oracle import coracle
    return coracle.test_field(threads=8)


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True)).cuda()


def message(e, npairs):
    return MALFORMED % e.bad if e.kind == "param" else COUNT % npairs


# ---- what the objects of one call must give ---------------------------------------------------
@functools.lru_cache(maxsize=None)
def wanted(which, session=False):
    """(objects, pair counts, expected mag (T, 2, 16) and neg (T, 2), per pair: its object or -1
    where the object is refused and its rows unspecified)."""
    objs = EC.objects(which, session)
    counts = [o.npairs for o in objs]
    vals, signs, owner = [], [], []
    for k, o in enumerate(objs):
        d = EC.diffs_of(o.expect.pairs) if o.expect.pairs is not None else [(0, 0)] * (2 * o.npairs)
        assert len(d) == 2 * o.npairs
        vals += [m for m, _ in d]
        signs += [s for _, s in d]
        owner += [k if o.expect.pairs is not None else -1] * o.npairs
    mag = FC.arr(vals).reshape(-1, 2, 16)
    neg = np.array(signs, np.uint8).reshape(-1, 2)
    for a in (mag, neg):
        a.setflags(write=False)
    assert any(o.clean for o in objs) and any(o.expect.kind == "param" for o in objs)
    return objs, counts, mag, neg, np.array(owner, np.int64)


def check_verdicts(objs, bad, tag):
    got = [int(x) for x in bad]
    wrong = [(o.name, g, o.expect.bad) for o, g in zip(objs, got) if g != o.expect.bad]
    assert len(got) == len(objs) and not wrong, "%s: %d of %d verdicts differ (name, got, wanted): %r" % (
        tag, len(wrong), len(objs), wrong[:12])


def check_rows(objs, owner, got_mag, got_neg, mag, neg, tag):
    """Accepted objects' magnitudes and sign bytes equal parse_pairs'; every clean object is bit-exact."""
    differ = ((np.asarray(got_mag) != mag).any(axis=(1, 2)) | (np.asarray(got_neg) != neg).any(axis=1)) & (owner >= 0)
    names = sorted({objs[int(k)].name for k in owner[differ]})
    assert not names, "%s: %d accepted objects decode to other values: %r" % (tag, len(names), names[:12])


def check_host_status(objs, status, tag):
    """AMPH_E_PARAM when any text is refused, naming the first such object, its offset and how many."""
    st, msg = status
    refused = [k for k, o in enumerate(objs) if o.expect.kind != "ok"]
    first = next(k for k in refused if objs[k].expect.kind == "param")
    assert st == E_PARAM and ("object %d: " % first + MALFORMED % objs[first].expect.bad) in msg, (tag, st, msg)
    assert "(%d of %d texts refused)" % (len(refused), len(objs)) in msg, (tag, msg)


def run_packed(mode):
    objs, counts, mag, neg, owner = wanted(EVERYTHING)
    assert {c.cls for c, _ in EC.catalogue(EVERYTHING)} == set(EC.CLASSES)
    got_mag, got_neg, bad, status = decode("host_packed" if mode == "host" else "device_packed",
                                           [o.text for o in objs], counts, fill=HOSTILE)
    check_verdicts(objs, bad, "packed/" + mode)
    check_rows(objs, owner, got_mag, got_neg, mag, neg, "packed/" + mode)
    if mode == "host":
        check_host_status(objs, status, "packed")


def run_batch(mode):
    objs, counts, mag, neg, owner = wanted("EDGE+PAIRS")
    got_mag, got_neg, bad, status = decode("host_batch", [o.text for o in objs], counts)
    check_verdicts(objs, bad, "batch")
    check_rows(objs, owner, got_mag, got_neg, mag, neg, "batch")
    check_host_status(objs, status, "batch")


# ---- amph_exchange_decode: one text a call ----------------------------------------------------
def run_single_device():
    """FULL, one device-mode call per case, each with its own verdict word and no host wait
    between; then the diagonal with every text 0, 1 and 15 bytes off a 16-byte boundary (device
    mode takes any text pointer)."""
    import torch
    ctx = _ctx()
    full = EC.catalogue("FULL")
    runs = [(c, e, 0) for c, e in full] + [(c, e, mis) for c, e in EC.diagonal() for mis in EC.ALIGN]
    stride = lambda n: -(-(n + 16) // 256) * 256  # noqa: E731 -- every text starts 256-aligned, plus its misalignment
    at, starts = 0, []
    for c, _, mis in runs:
        starts.append(at + mis)
        at += stride(len(c.text))
    buf = np.frombuffer((HOSTILE * (at // len(HOSTILE) + 1))[:at], np.uint8).copy()
    for (c, _, _), a in zip(runs, starts):
        buf[a:a + len(c.text)] = np.frombuffer(c.text, np.uint8)
    texts = dev(buf)
    assert texts.data_ptr() % 256 == 0
    results = [ctx.exchange_decode(texts[a:a + len(c.text)], c.npairs) for (c, _, _), a in zip(runs, starts)]
    torch.cuda.synchronize()  # the one wait
    bad = torch.cat([b.reshape(1) for _, _, b in results]).cpu().numpy()
    got = [-1 if int(x) == NF else int(x) for x in bad]
    wrong = [(c.name, mis, g, e.bad) for (c, e, mis), g in zip(runs, got) if g != e.bad]
    assert not wrong, "single/device: %d of %d verdicts differ (name, misalignment, got, wanted): %r" % (
        len(wrong), len(runs), wrong[:12])
    mags = torch.stack([m for m, _, _ in results[:len(full)]]).cpu().numpy()
    negs = torch.stack([g for _, g, _ in results[:len(full)]]).cpu().numpy()
    values = []
    for k, (c, e, mis) in enumerate(runs):
        if e.pairs is None:
            continue
        d = EC.diffs_of(e.pairs)
        m, g = (mags[k], negs[k]) if k < len(full) else (results[k][0].cpu().numpy(), results[k][1].cpu().numpy())
        if not (np.array_equal(m, FC.arr([v for v, _ in d]).reshape(-1, 2, 16)) and
                np.array_equal(g, np.array([s for _, s in d], np.uint8).reshape(-1, 2))):
            values.append((c.name, mis))
    assert not values, "single/device: %d accepted texts decode to other values: %r" % (len(values), values[:12])


def run_single_host():
    """One case of every class and place and every digit count, each text at pointer offsets 0, 1
    and 15 from a 16-byte boundary: status, verdict and message, the same at all three."""
    L, ctx = _L(), _ctx()
    wrong = []
    for c, e in EC.diagonal():
        n = len(c.text)
        store = np.zeros(n + 48, np.uint8)
        for mis in EC.ALIGN:
            a = (-store.ctypes.data) % 16 + mis
            store[:] = 0x3A  # colons around the text
            store[a:a + n] = np.frombuffer(c.text, np.uint8)
            mag, neg = np.zeros((c.npairs + 1, 2, 16), np.uint8), np.zeros((c.npairs + 1, 2), np.uint8)
            bad = C.c_int64(-1)
            st = L.lib.amph_exchange_decode(ctx._h, store.ctypes.data + a, n, c.npairs, mag.ctypes.data,
                                            neg.ctypes.data, C.byref(bad), 0, None)
            msg = L.lib.amph_last_error().decode() if st != OK else ""
            ok = st == STATUS[e.kind] and bad.value == e.bad and (e.kind == "ok" or message(e, c.npairs) in msg)
            if ok and e.pairs is not None:
                d = EC.diffs_of(e.pairs)
                ok = np.array_equal(mag[:c.npairs], FC.arr([v for v, _ in d]).reshape(-1, 2, 16)) and \
                    np.array_equal(neg[:c.npairs], np.array([s for _, s in d], np.uint8).reshape(-1, 2))
            if not ok:
                wrong.append((c.name, mis, st, bad.value, msg, (STATUS[e.kind], e.bad)))
    assert not wrong, "single/host: %d calls differ (name, misalignment, status, verdict, message, wanted): %r" % (
        len(wrong), wrong[:8])


def run_single(mode):
    run_single_host() if mode == "host" else run_single_device()


# ---- the sessions ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def party_inputs(words):
    """Party 0's tuples for `words` words and what the oracle opens from them."""
    F = _F()
    shares = F.synth_words(seed=100, count=2 * words).reshape(words, 32)
    masks = F.synth_words(seed=200, count=4 * words).reshape(2 * words, 32)
    triples = F.synth_words(seed=300, count=12 * words).reshape(2 * words, 96)
    pre = F.odo_pre(shares, 32, masks, triples)
    for a in (shares, masks, triples):
        a.setflags(write=False)
    return shares, masks, triples, pre


def oracle_fields(words, mag, neg):
    """(y, r, v, w, u) of party 0 (player 0) of two, its partner's diffs being mag / neg."""
    F = _F()
    _, _, triples, pre = party_inputs(words)
    opened = F.recombine_diffs([pre[3], np.ascontiguousarray(mag)], [pre[4], np.ascontiguousarray(neg)])
    w, u = F.odo_post(opened, triples, True)
    return pre[0], pre[1], pre[2], w, u


def b64(rows):
    return base64.b64encode(np.ascontiguousarray(rows).tobytes())


def run_party(mode):
    """The diagonal through a session of matching size: one partner text a session."""
    import torch
    import amphora_amd as A
    L, ctx = _L(), _ctx()
    cases = [(c, e) for c, e in EC.diagonal() if c.npairs >= 2 and c.npairs % 2 == 0]
    assert {c.cls for c, _ in cases} >= {"EDGE", "NUMBERS", "PAIRS", "ACCEPTED"}
    assert {c.role[0] for c, e in cases if c.role and e.kind == "ok"} == set(range(1, 40))
    assert {e.kind for _, e in cases} == {"ok", "param", "len"}
    wrong = []
    for c, e in cases:
        W = c.npairs // 2
        shares, masks, triples, pre = party_inputs(W)
        want = None
        if e.pairs is not None:
            d = EC.diffs_of(e.pairs)
            want = oracle_fields(W, FC.arr([v for v, _ in d]).reshape(-1, 2, 16),
                                 np.array([s for _, s in d], np.uint8).reshape(-1, 2))
        a = np.frombuffer(c.text, np.uint8)
        if mode == "host":
            s = ctx.party_begin(shares, 32, masks, triples, 2, want_yrv=False)
            bad = C.c_int64(-1)
            st = L.lib.amph_party_partner(s._h, 1, L._ptr(a), a.size, C.byref(bad))
            msg = L.lib.amph_last_error().decode() if st != OK else ""
            ok = st == STATUS[e.kind] and bad.value == e.bad and (e.kind == "ok" or message(e, c.npairs) in msg)
            if e.kind == "ok":
                w, u = s.finish(True)
                ok = ok and np.array_equal(w, want[3]) and np.array_equal(u, want[4])
            else:  # the slot stays free
                with pytest.raises(A.AmphoraNativeError, match="partner slot 1's interimValues text is missing"):
                    s.finish(True)
            if not ok:
                wrong.append((c.name, st, bad.value, msg, (STATUS[e.kind], e.bad)))
        else:
            s = ctx.party_begin_dev(dev(shares), 32, dev(masks), dev(triples), 2)
            word = s.partner(1, dev(a))
            fields = s.finish_b64(True)
            torch.cuda.synchronize()
            got = [f.cpu().numpy().tobytes() for f in fields]
            v = int(word.item())
            if e.kind == "ok":
                ok = v == NF and got == [b64(x) for x in want]
            else:  # a device session is poisoned
                ok = v == e.bad and all(g[:4] == b"!!!!" for g in got)
            if not ok:
                wrong.append((c.name, v, e.bad, [g[:8] for g in got]))
        s.close()
    assert not wrong, "party/%s: %d of %d sessions differ: %r" % (mode, len(wrong), len(cases), wrong[:8])


def run_parties(mode):
    """EDGE x PLACES and PAIRS as one party's K partner texts, two pairs a word."""
    import torch
    ctx = _ctx()
    objs, counts, mag, neg, owner = wanted("EDGE+PAIRS", True)
    words = [p // 2 for p in counts]
    woff = offsets(words)
    T = int(woff[-1])
    assert 0 in words and max(words) > 90 and len(objs) > 2000
    shares, masks, triples, pre = party_inputs(T)
    want = oracle_fields(T, mag, neg)
    refused = np.array([o.expect.kind != "ok" for o in objs])
    texts = [o.text for o in objs]
    rows_ok = np.repeat(~refused, words)

    def check_fields(got, rej, tag):
        differ = []
        for k, o in enumerate(objs):
            a, b = int(woff[k]), int(woff[k + 1])
            if refused[k]:
                if b > a and not all(f[:4] == b"!!!!" for f in got[k]):
                    differ.append((o.name, "not poisoned", got[k][0][:8]))
            elif got[k] != [b64(x[a:b]) for x in want]:
                differ.append((o.name, "fields"))
        assert not differ, "%s: %d objects' fields differ: %r" % (tag, len(differ), differ[:8])
        if rej is not None:
            flagged = [o.name for k, o in enumerate(objs) if bool(rej[k]) != bool(refused[k]) and words[k]]
            assert not flagged, (tag, flagged[:8])

    if mode == "host":
        for finish in ("finish_b64", "finish"):
            s = ctx.parties_begin(shares, 32, masks, triples, woff, 2, want_yrv=False)
            bad, st = s.partner(1, texts, status=True)
            check_verdicts(objs, bad, "parties/host")
            assert st == E_PARAM, st
            if finish == "finish":
                w, u = s.finish(True)
                differ = (((w != want[3]).any(axis=1) | (u != want[4]).any(axis=1)) & rows_ok).nonzero()[0]
                names = sorted({objs[int(np.searchsorted(woff, r, "right")) - 1].name for r in differ})
                assert not names, "parties/host: %d accepted objects' w, u differ: %r" % (len(names), names[:8])
            else:
                fields, rej = s.finish_b64(True)
                check_fields(s.split_fields(fields), rej, "parties/host")
            s.close()
        return
    s = ctx.parties_begin_dev(dev(shares), 32, dev(masks), dev(triples), woff, 2)
    buf, lens = s.pack_texts(texts)
    bad = s.partner(1, dev(buf), dev(lens.view(np.int64)))
    fields = s.finish_b64(True)
    torch.cuda.synchronize()
    bad = bad.cpu().numpy()
    check_verdicts(objs, np.where(bad == NF, -1, bad), "parties/device")
    check_fields(s.split_fields([f.cpu().numpy() for f in fields]), None, "parties/device")
    s.close()


RUN = {"single": run_single, "packed": run_packed, "batch": run_batch, "party": run_party, "parties": run_parties}


def form_parameters():
    return [(e.form, mode) for e in EC.MATRIX.values() for mode in e.modes]


@pytest.mark.parametrize("form,mode", form_parameters())
def test_the_catalogue_through(form, mode):
    assert sorted(RUN) == sorted(FORMS)
    RUN[form](mode)
