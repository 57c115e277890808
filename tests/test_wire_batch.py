"""Many secrets straight from their base64 wire texts, on the GPU
(include/amphora_wire_batch.h): amph_recombine_verify_b64_packed /
amph_mask_input_b64_packed in host and device mode and the gather forms
amph_recombine_verify_b64_batch / amph_mask_input_b64_batch.

Every expected value comes from the C oracle on the decoded fields of each
object by itself (the texts are Python's base64 of those fields) -- never
from the library's single wire-text call.  The table's objects cover the
three padding classes (1, 2, 3 words), the 192-word tile's edges, an object of
several fast tiles that is not the first, and empty objects at both ends.
"""
import base64
import functools
import json
import uuid

import numpy as np
import pytest

from oracle import amphora_oracle as O
from oracle import coracle
from tests import extent_cases as X
from tests import field_cases as FC

pytestmark = pytest.mark.gpu

P, R, RINV = O.TEST_PRIME, O.TEST_R, O.TEST_RINV
NO_FAIL = 0x7F7F7F7F7F7F7F7F
OK, E_VERIFY, E_PARAM = 0, 1, 3
SIZES = [0, 1, 2, 3, 191, 192, 193, 383, 384, 385, 577, 1000, 0]  # 4,212 words
# object -> faulted local words: the single word of the 1-word object, word 0,
# a last word, words 191 / 192 either side of a tile edge (in the 385-word
# object twice: the smaller index wins), the last word of the largest object
FAULTS = {1: [0], 4: [0], 6: [192], 9: [191, 300], 10: [192], 11: [999]}
FAULTS_2 = {9: [5], 10: [400], 3: [2]}  # a second pass for AMPH_F_ACCUMULATE
FORMS = ["packed_host", "packed_device", "batch"]


def nchars_of(words):
    return 4 * ((16 * words + 2) // 3)


def slot_of(words):
    return -(-nchars_of(words) // 16) * 16


@functools.lru_cache(maxsize=None)
def _field(pid):
    pr = FC.BY_ID[pid]
    return pr, coracle.Field(pr.p, pr.r, pr.rinv, threads=4)


class Batch:
    """One batch: per-object ODOs from its own synth_odos call, the faults
    applied, the oracle's results and the base64 texts, object by object."""

    def __init__(self, n, pid, sizes, faults, seed):
        pr, F = _field(pid)
        self.n, self.pid, self.sizes = n, pid, list(sizes)
        self.objects, self.secrets, self.y, self.masked, self.ff, self.texts, self.records = [], [], [], [], [], [], []
        for o, W in enumerate(sizes):
            if W == 0:
                e = np.zeros((0, 16), np.uint8)
                odos, sec, y, m, ff = [tuple(e.copy() for _ in range(5)) for _ in range(n)], e.copy(), e.copy(), e.copy(), -1
            else:
                odos, _ = F.synth_odos(seed=seed + 31 * o, n=n, W=W, noncanon_permille=200)
                odos = [tuple(np.ascontiguousarray(f).copy() for f in p) for p in odos]
                for i in faults.get(o, []):
                    odos[n - 1][3][i, 0] ^= 1  # <w> of the last party: w != y r at word i
                sec = F.synth_words(seed=seed + 31 * o + 7, count=W, mont=False)
                y, ff = F.recombine_verify(odos)
                m, mff = F.mask_input(sec, odos)
                assert ff == mff == (min(faults[o]) if o in faults else -1), "the fixture's faults"
            self.objects.append(odos)
            self.secrets.append(sec)
            self.y.append(y)
            self.masked.append(m)
            self.ff.append(int(ff))
            self.texts.append([[base64.b64encode(f.tobytes()) for f in p] for p in odos])
            self.records.append(np.frombuffer(b"".join(base64.b64encode(w.tobytes()) for w in m), np.uint8)
                                .reshape(-1, 24))
        self.woff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
        self.packed_secrets = np.ascontiguousarray(np.concatenate(self.secrets))
        for a in (self.woff, self.packed_secrets):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def batch(n, pid="test", faults="none"):
    return Batch(n, pid, SIZES, {"none": {}, "faults": FAULTS, "faults2": FAULTS_2}[faults], seed=2000 + n)


def layout(sizes, kind):
    """(text_offsets, buffer length).  dense: amph_wire_slot_chars strides;
    sparse: a first slot at 48 and a gap of 0-4 units after every slot.  The
    buffers end at the last slot offset or the last text's end, whichever is
    later -- for a table whose last object is not empty, exactly at the last
    character."""
    toff, at = [], 48 if kind == "sparse" else 0
    for o, W in enumerate(sizes):
        toff.append(at)
        at += slot_of(W) + (16 * ((7 * o + 3) % 5) if kind == "sparse" else 0)
    return np.array(toff, np.uint64), max(toff[-1], toff[-1] + nchars_of(sizes[-1]))


def buffers(texts, sizes, toff, nchars, fill=b"!"):
    """Per party the five field buffers: `fill` everywhere, each object's text
    at its slot."""
    n = len(texts[0]) if texts else 1
    out = []
    for j in range(n):
        fs = []
        for k in range(5):
            buf = np.frombuffer((fill * (nchars // len(fill) + 1))[:nchars], np.uint8).copy()
            for o, W in enumerate(sizes):
                t = texts[o][j][k]
                assert len(t) == nchars_of(W)
                buf[int(toff[o]):int(toff[o]) + len(t)] = np.frombuffer(t, np.uint8)
            fs.append(buf)
        out.append(tuple(fs))
    return out


@pytest.fixture(scope="module")
def A():
    import amphora_amd
    return amphora_amd


@functools.lru_cache(maxsize=None)
def _ctx(pid, multi=False):
    import amphora_amd
    pr = FC.BY_ID[pid]
    return amphora_amd.Context(pr.p, pr.r, pr.rinv, devices=[0, 0] if multi else None)


def _dev(x):
    import torch
    x = np.array(x, copy=True)
    return torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).cuda()


def _host(v):
    import torch
    torch.cuda.synchronize()
    v = v.cpu().numpy()
    return np.where(v == NO_FAIL, -1, v) if v.dtype == np.int64 else v


def _split(a, woff):
    return [np.asarray(a)[int(woff[o]):int(woff[o + 1])] for o in range(len(woff) - 1)]


def run(ctx, b, form, masked, texts=None, kind="dense", fill=b"!"):
    """One call in one form -> dict(y | m16, m24, ff, bad, status, message),
    outputs split per object, verdicts as host values (-1 = clean)."""
    texts = b.texts if texts is None else texts
    if form == "batch":
        if masked:
            m16, m24, ff, bad, st = ctx.mask_input_b64_batch(texts, b.sizes, b.secrets, records=True, raw=True,
                                                            status=True)
            return dict(m16=m16, m24=m24, ff=ff, bad=bad, status=st[0], message=st[1])
        y, ff, bad, st = ctx.recombine_verify_b64_batch(texts, b.sizes, status=True)
        return dict(y=y, ff=ff, bad=bad, status=st[0], message=st[1])
    toff, nchars = layout(b.sizes, kind)
    bufs = buffers(texts, b.sizes, toff, nchars, fill)
    woff, sec = b.woff, b.packed_secrets
    if form == "packed_device":
        bufs = [tuple(_dev(f) for f in p) for p in bufs]
        woff, toff, sec = _dev(woff), _dev(toff), _dev(sec)
    if masked:
        m16, m24, ff, bad, st = ctx.mask_input_b64_packed(bufs, woff, toff, sec, records=True, raw=True, status=True)
        res = dict(m16=_split(_host(m16) if form == "packed_device" else m16, b.woff),
                   m24=_split(_host(m24) if form == "packed_device" else m24, b.woff))
    else:
        y, ff, bad, st = ctx.recombine_verify_b64_packed(bufs, woff, toff, status=True)
        res = dict(y=_split(_host(y) if form == "packed_device" else y, b.woff))
    if form == "packed_device":
        ff, bad = _host(ff), _host(bad)
    res.update(ff=ff, bad=bad, status=st[0], message=st[1])
    return res


def check(b, res, masked, bad=None, device=False):
    """Outputs and verdicts against the oracle; bad = {object: index}: those
    objects' outputs are unspecified (and in device mode their first_fail)."""
    bad = bad or {}
    K = len(b.sizes)
    assert list(res["bad"]) == [bad.get(o, -1) for o in range(K)]
    want_ff = [-1 if o in bad else b.ff[o] for o in range(K)]
    got_ff = [want_ff[o] if (device and o in bad) else int(res["ff"][o]) for o in range(K)]
    assert got_ff == want_ff
    for o in range(K):
        if o in bad:
            continue
        if masked:
            assert res["m16"][o].shape == b.masked[o].shape and np.array_equal(res["m16"][o], b.masked[o]), o
            assert res["m24"][o].shape == b.records[o].shape and np.array_equal(res["m24"][o], b.records[o]), o
        else:
            assert res["y"][o].shape == b.y[o].shape and np.array_equal(res["y"][o], b.y[o]), o


# ---------------------------------------------------------------- honest and MAC faults
@pytest.mark.parametrize("masked", [False, True], ids=["rv", "mask"])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n,pid", [(1, "test"), (2, "test"), (3, "test"), (4, "test"), (5, "test"), (2, "m89"),
                                   (3, "m89")])  # 5 parties, and 3 below 2^127, take the run-time party loop
def test_honest_batch_matches_the_oracle(n, pid, form, masked):
    b = batch(n, pid)
    res = run(_ctx(pid), b, form, masked)
    assert res["status"] == OK
    check(b, res, masked, device=form == "packed_device")


@pytest.mark.parametrize("masked", [False, True], ids=["rv", "mask"])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n,pid", [(1, "test"), (2, "test"), (3, "test"), (4, "test"), (5, "test"), (2, "m89")])
def test_mac_faults_keep_to_their_objects(n, pid, form, masked):
    b = batch(n, pid, "faults")
    assert [o for o, f in enumerate(b.ff) if f >= 0] == sorted(FAULTS) and b.ff[9] == 191
    res = run(_ctx(pid), b, form, masked)
    check(b, res, masked, device=form == "packed_device")  # failed objects' words equal the oracle's too
    if form != "packed_device":
        assert res["status"] == E_VERIFY
        assert "object 1 at word 0" in res["message"] and "(6 of 13 objects failed)" in res["message"]


# ---------------------------------------------------------------------- bad characters
def _bad_cases(n):
    """[(object, party, field, offset, character)] and the expected verdicts."""
    last = n - 1
    nc = {o: nchars_of(W) for o, W in enumerate(SIZES)}
    cases = [
        (11, last, 4, 0, b"!"),              # the first character of an object
        (9, 0, 0, nc[9] - 3, b"*"),          # its last character before the '==' padding
        (1, last, 4, 22, b"A"),              # a non-'=' where padding is required
        (7, 0, 0, nc[7] - 6, b"="),          # an '=' in a non-final group
        (10, min(1, last), 2, 5000, b"\xff"),  # the fast path of a middle tile
        (6, 0, 1, 7, b"-"),                  # with a MAC fault in the same object (FAULTS[6])
        (10, last, 4, 12000, b"!"),          # a later field of the same object: the smaller index wins
    ]
    exp = {}
    for o, j, k, off, _ in cases:
        v = (5 * j + k) * nc[o] + off
        exp[o] = min(exp.get(o, v), v)
    return cases, exp


def _with_bad_chars(b, cases):
    texts = [[list(p) for p in obj] for obj in b.texts]
    for o, j, k, off, ch in cases:
        t = bytearray(texts[o][j][k])
        assert t[off:off + 1] != ch
        t[off:off + 1] = ch
        texts[o][j][k] = bytes(t)
    return texts


@pytest.mark.parametrize("masked", [False, True], ids=["rv", "mask"])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_bad_characters_report_their_own_object(n, form, masked):
    b = batch(n, "test", "faults")
    assert SIZES[9] * 16 % 3 == 1 and SIZES[1] * 16 % 3 == 1 and SIZES[7] * 16 % 3 == 2  # '==', '==', '='
    cases, exp = _bad_cases(n)
    res = run(_ctx("test"), b, form, masked, texts=_with_bad_chars(b, cases), kind="sparse")
    check(b, res, masked, bad=exp, device=form == "packed_device")
    if form != "packed_device":
        # a bad character outranks the MAC failure of object 4; objects 1, 6, 9, 10 and 11 have both
        assert res["status"] == E_PARAM and int(res["ff"][6]) == -1 and int(res["ff"][4]) == 0
        j, k, off = n - 1, 4, 22
        assert res["message"].startswith("object 1: Illegal base64 character at index %d of party %d's uShares"
                                         % (off, j)), res["message"]
        assert "(6 of 13 objects" in res["message"]
        A = __import__("amphora_amd")
        assert A._lib.wire_bad_char_message(exp[1], 1) == res["message"][len("object 1: "):res["message"].index(" (")]


# -------------------------------------------------------------------------- gap bytes
def _guarded_call(L, ctx, b, sizes, texts, kind, fill, device, masked):
    """The packed call over buffers that end where layout() says, every array
    inside the guard bands of tests/extent_cases.py's arena."""
    K, n = len(sizes), b.n
    toff, nchars = layout(sizes, kind)
    bufs = buffers(texts, sizes, toff, nchars, fill)
    woff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    T = int(woff[-1])
    main = X.Arena(device)
    g_in = {(j, k): main.add("t%d%d" % (j, k), X.B64, data=bufs[j][k], fill="hostile") for j in range(n) for k in range(5)}
    g_w = main.add("woff", X.OFFS, data=woff, fill="hostile")
    g_t = main.add("toff", X.OFFS, data=toff, fill="hostile")
    g_s = main.add("secrets", X.WORD, data=np.concatenate(b.secrets[:K]), fill="hostile") if masked else None
    g_16 = main.add("out16", X.WORD, n=16 * T)
    g_24 = main.add("out24", X.WORD, n=24 * T) if masked else None
    g_ff = main.add("ff", X.VERDICT, n=8 * K)
    g_bad = main.add("bad", X.VERDICT, n=8 * K)
    main.commit()
    arr = (L._AmphOdoB64 * n)()
    for j in range(n):
        arr[j] = L._AmphOdoB64(*[g_in[(j, k)].ptr for k in range(5)], nchars)
    flags = X.F_DEVICE if device else 0
    if masked:
        st = L.lib.amph_mask_input_b64_packed(ctx._h, arr, n, g_w.ptr, g_t.ptr, K, g_s.ptr, g_16.ptr, g_24.ptr,
                                              g_ff.ptr, g_bad.ptr, flags, None)
    else:
        st = L.lib.amph_recombine_verify_b64_packed(ctx._h, arr, n, g_w.ptr, g_t.ptr, K, g_16.ptr, g_ff.ptr,
                                                    g_bad.ptr, flags, None)
    if device:
        import torch
        torch.cuda.synchronize()
    main.fetch()
    for g in main.items:
        (g.check_untouched if g in (g_16, g_24, g_ff, g_bad) else g.check_unchanged)()
    v = lambda g: np.frombuffer(g.payload(), np.int64)  # noqa: E731
    none = NO_FAIL if device else -1
    assert st == OK and list(v(g_ff)) == [none] * K and list(v(g_bad)) == [none] * K, (st, L.lib.amph_last_error())
    return g_16.payload(), g_24.payload() if masked else None


@pytest.mark.parametrize("masked", [False, True], ids=["rv", "mask"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("table", ["13", "12"])
def test_gap_bytes_are_never_read(A, device, masked, table):
    """Dense and sparse slots with '!', '=' and 0xFF between and after the
    texts give the clean dense result; table "12" drops the trailing empty
    object, so its buffers END at the last text's last character, inside the
    arena's hostile bands, which stay intact."""
    b = batch(2)
    K = int(table)
    sizes, texts = SIZES[:K], b.texts[:K]
    want16 = np.concatenate((b.masked if masked else b.y)[:K]).tobytes()
    want24 = np.concatenate(b.records[:K]).tobytes()
    if K == 12:
        toff, nchars = layout(sizes, "dense")
        assert nchars == int(toff[-1]) + nchars_of(1000) and nchars % 16 == 8
    for kind, fill in [("dense", b"!"), ("sparse", b"!"), ("sparse", b"="), ("sparse", b"\xff"), ("sparse", b"!=\xff")]:
        o16, o24 = _guarded_call(A._lib, _ctx("test"), b, sizes, texts, kind, fill, device, masked)
        assert o16 == want16, (kind, fill)
        assert not masked or o24 == want24, (kind, fill)


# ----------------------------------------------------------- accumulate, multi-device
@pytest.mark.parametrize("masked", [False, True], ids=["rv", "mask"])
def test_accumulate_min_combines_per_object(masked):
    import torch
    ctx = _ctx("test")
    b1, b2 = batch(2, "test", "faults"), batch(2, "test", "faults2")
    cases = [(5, 1, 3, 40, b"!"), (9, 0, 0, 9, b"?")]
    toff, nchars = layout(SIZES, "dense")
    woff, dt = _dev(b1.woff), _dev(toff)
    ff = torch.full((13,), NO_FAIL, dtype=torch.int64, device="cuda")
    bad = torch.full((13,), NO_FAIL, dtype=torch.int64, device="cuda")
    for b, texts in ((b1, b1.texts), (b2, _with_bad_chars(b2, cases))):
        bufs = [tuple(_dev(f) for f in p) for p in buffers(texts, SIZES, toff, nchars)]
        if masked:
            ctx.mask_input_b64_packed(bufs, woff, dt, _dev(b.packed_secrets), first_fail=ff, bad_char=bad,
                                      accumulate=True)
        else:
            ctx.recombine_verify_b64_packed(bufs, woff, dt, first_fail=ff, bad_char=bad, accumulate=True)
    want = [min(x for x in (b1.ff[o], b2.ff[o]) if x >= 0) if max(b1.ff[o], b2.ff[o]) >= 0 else -1 for o in range(13)]
    got_ff, got_bad = _host(ff), _host(bad)
    assert list(got_bad) == [(5 * 1 + 3) * nchars_of(192) + 40 if o == 5 else 9 if o == 9 else -1 for o in range(13)]
    # objects 5 and 9 did not parse in the second call: its verdict for them is unspecified
    assert [got_ff[o] for o in range(13) if o not in (5, 9)] == [want[o] for o in range(13) if o not in (5, 9)]
    assert want[10] == 192 and want[3] == 2 and want[11] == 999
    # without the flag the second call's own verdicts replace the first's
    bufs = [tuple(_dev(f) for f in p) for p in buffers(b2.texts, SIZES, toff, nchars)]
    if masked:
        ctx.mask_input_b64_packed(bufs, woff, dt, _dev(b2.packed_secrets), first_fail=ff, bad_char=bad)
    else:
        ctx.recombine_verify_b64_packed(bufs, woff, dt, first_fail=ff, bad_char=bad)
    assert list(_host(ff)) == b2.ff and list(_host(bad)) == [-1] * 13


@pytest.mark.parametrize("masked", [False, True], ids=["rv", "mask"])
@pytest.mark.parametrize("form", FORMS)
def test_multi_device_context_runs_on_its_first_device(form, masked):
    b = batch(2, "test", "faults")
    res = run(_ctx("test", multi=True), b, form, masked)
    check(b, res, masked, device=form == "packed_device")


# ------------------------------------------------- small and staged paths, copy count
@pytest.mark.parametrize("masked", [False, True], ids=["rv", "mask"])
def test_small_and_staged_host_paths_and_copies_do_not_grow_with_k(A, masked):
    """The 13-object table at 1 party fits the small-call arena (no copies:
    the kernel works in the arena); 64 objects of 1,000 words x 2 parties are
    far above AMPH_SMALL_BYTES and take the staged path, whose copies are one
    image in and one out -- for 64 objects as for 16 -- and one kernel launch."""
    ctx = A.Context(P, R, RINV)
    b = batch(1)
    res = run(ctx, b, "batch", masked)
    check(b, res, masked)
    assert ctx.wire_batch_copies() == 0
    big = Batch(2, "test", [1000] * 64, {17: [999], 63: [0]}, seed=77)
    assert 16 * 10 * nchars_of(1000) > (2 << 20)  # both counts are above the default AMPH_SMALL_BYTES
    deltas = []
    for K in (64, 16):
        sub = dict(texts=big.texts[:K], sizes=big.sizes[:K], secrets=big.secrets[:K])
        c0, l0 = ctx.wire_batch_copies(), ctx.stats()["kernel_launches"]
        if masked:
            m16, m24, ff, bad = ctx.mask_input_b64_batch(sub["texts"], sub["sizes"], sub["secrets"], raw=True)
            assert all(np.array_equal(m16[o], big.masked[o]) and np.array_equal(m24[o], big.records[o])
                       for o in range(K))
        else:
            y, ff, bad = ctx.recombine_verify_b64_batch(sub["texts"], sub["sizes"])
            assert all(np.array_equal(y[o], big.y[o]) for o in range(K))
        assert list(ff) == big.ff[:K] and list(bad) == [-1] * K
        deltas.append((ctx.wire_batch_copies() - c0, ctx.stats()["kernel_launches"] - l0))
    assert deltas == [(2, 1), (2, 1)]


# ---------------------------------------------------------------------- client mirrors
def test_client_mirrors_give_the_single_functions_outcomes(A):
    """6 secrets with one MAC fault, one bad character and one irregular
    secret: entry by entry what verify_vss_json / create_masked_input_json
    give, exception type and text included."""
    from amphora_amd import client, wire
    ctx = _ctx("test")
    util = client.SecretShareUtil(ctx)
    b = batch(2, "test", "faults")
    pick = [3, 5, 6, 7, 8, 11]  # 6: MAC fault at word 192; 11: MAC fault at 999
    sids = [uuid.UUID(int=1000 + o) for o in pick]

    def bodies(o, vss, texts=None):
        out = []
        for j in range(b.n):
            odo = A.OutputDeliveryObject(*[f.tobytes() for f in b.objects[o][j]])
            d = json.loads(wire.vss_to_json(ctx, uuid.UUID(int=o), [], odo, pretty=False) if vss
                           else wire.odo_to_json(ctx, odo))
            for k, name in enumerate(("secretShares", "rShares", "vShares", "wShares", "uShares")):
                assert d[name].encode() == b.texts[o][j][k]
                if texts:
                    d[name] = texts[j][k].decode("latin-1")
            out.append(json.dumps(d, separators=(",", ":")))
        return out

    bad_texts = [list(p) for p in b.texts[7]]
    bad_texts[1][2] = bad_texts[1][2][:100] + b"!" + bad_texts[1][2][101:]  # object 7: a bad character
    for vss in (True, False):
        lists = [bodies(o, vss, bad_texts if o == 7 else None) for o in pick]
        lists[1] = lists[1] + [lists[1][0]]  # object 5 with a third party: irregular, and its MACs fail
        secrets = [A.Secret.of([], client.unpack(b.secrets[o]), secret_id=sids[i]) for i, o in enumerate(pick)]
        if not vss:
            secrets[4] = A.Secret.of([], client.unpack(b.secrets[8])[:100], secret_id=sids[4])  # fewer secrets: irregular
        singles = []
        for i in range(6):
            try:
                singles.append(client.verify_vss_json(util, lists[i], sids[i]) if vss
                               else client.create_masked_input_json(util, secrets[i], lists[i]))
            except Exception as e:  # noqa: BLE001
                singles.append(e)
        got = client.verify_vss_json_batch(util, lists, sids) if vss \
            else client.create_masked_inputs_from_bodies(util, secrets, lists)
        assert len(got) == 6
        for i, (g, s) in enumerate(zip(got, singles)):
            if isinstance(s, Exception):
                assert type(g) is type(s) and str(g) == str(s), (i, g, s)
            else:
                assert g == s, i
        assert isinstance(got[2], A.IntegrityVerificationException) and isinstance(got[5], A.IntegrityVerificationException)
        assert isinstance(got[3], A.AmphoraClientException) and "index 100 of party 1's vShares" in str(got[3])
        assert isinstance(got[1], A.IntegrityVerificationException)  # through the single function
        # and the values themselves come from the oracle
        if vss:
            assert got[0] == (sids[0], [], client.unpack(b.y[3]))
        else:
            assert got[0] == wire.records_to_masked_input_json(sids[0], b.records[3], [])
            assert json.loads(got[4])["data"][99]["value"] == b.records[8][99].tobytes().decode()
