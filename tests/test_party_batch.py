"""Many Output Delivery requests of one party in one device-resident session
(amph_parties_*, include/amphora_party_batch.h) against the C oracle, for
every party of an N-party exchange: the packed y / r / v and every object's
interimValues text after begin (the oracle's diffs formatted as Jackson
writes them), the packed w / u and every object's five base64 fields after
the partners' texts (recombineDiffs + multiplySharedSecrets on the oracle,
Python's base64).  Then the properties the batch form adds: per object the
bytes of K single amph_party_* sessions; objects in span form and in pair
order side by side; texts that end one character before, at and after a span
boundary; one faulty object that moves only itself; device mode with the
texts handed over on the device; and a launch count that does not depend on
K.  References are the oracle, Python ints, base64 and json -- another call
into the library only where "equals the single call" is the property.
"""
import base64
import functools
import re
import uuid

import numpy as np
import pytest

from oracle import amphora_oracle as O

P, R, RINV = O.TEST_PRIME, O.TEST_R, O.TEST_RINV
NO_FAILURE = 0x7F7F7F7F7F7F7F7F
OK, E_LEN, E_PARAM = 0, 2, 3
SPAN = 8192

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import amphora_amd as A
    return A.Context(P, R, RINV)


@pytest.fixture(scope="module")
def F():
    from oracle import coracle
    return coracle.test_field(threads=8)


def jackson_text(mag, neg) -> bytes:
    """The FactorPair JSON array of diffs (mag (P, 2, 16) LE, neg (P, 2))."""
    vals = []
    for k in range(mag.shape[0]):
        pair = []
        for j in range(2):
            x = int.from_bytes(mag[k, j].tobytes(), "little")
            pair.append(-x if neg[k, j] and x else x)
        vals.append('{"a":%d,"b":%d}' % tuple(pair))
    return ("[" + ",".join(vals) + "]").encode()


class Case:
    """n parties' packed inputs over the objects of `counts` words, and what
    the oracle makes of them (computed once per shape, never changed)."""

    def __init__(self, F, n, counts, stride=32, zero_objects=(), edit=None):
        self.n, self.counts, self.stride = n, list(counts), stride
        self.woff = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
        T = self.T = int(self.woff[-1])
        self.shares = [F.synth_words(seed=100 + j, count=T * stride // 16).reshape(T, stride) for j in range(n)]
        self.masks = [F.synth_words(seed=200 + j, count=4 * T).reshape(2 * T, 32) for j in range(n)]
        self.triples = [F.synth_words(seed=300 + j, count=12 * T).reshape(2 * T, 96) for j in range(n)]
        for o in zero_objects:  # triples whose a, b equal the words they are subtracted from: every diff is 0
            a, b = int(self.woff[o]), int(self.woff[o + 1])
            for j in range(n):
                t, s, m = self.triples[j], self.shares[j], self.masks[j]
                t[2 * a:2 * b:2, 0:16] = s[a:b, 0:16]
                t[2 * a:2 * b:2, 32:48] = m[2 * a:2 * b:2, 0:16]
                t[2 * a + 1:2 * b:2, 0:16] = m[2 * a + 1:2 * b:2, 0:16]
                t[2 * a + 1:2 * b:2, 32:48] = m[2 * a:2 * b:2, 0:16]
        if edit:
            edit(self)
        self.pre = [F.odo_pre(self.shares[j], stride, self.masks[j], self.triples[j]) for j in range(n)]
        for x in self.shares + self.masks + self.triples:
            x.setflags(write=False)
        self.F = F

    def obj(self, o):
        return int(self.woff[o]), int(self.woff[o + 1])

    def texts(self, j):
        """Party j's K texts as Jackson writes them."""
        mag, neg = self.pre[j][3], self.pre[j][4]
        return [jackson_text(mag[2 * a:2 * b], neg[2 * a:2 * b]) for a, b in map(self.obj, range(len(self.counts)))]

    @functools.lru_cache(maxsize=None)
    def wu(self, j):
        order = [j] + [k for k in range(self.n) if k != j]
        opened = self.F.recombine_diffs([self.pre[k][3] for k in order], [self.pre[k][4] for k in order])
        return self.F.odo_post(opened, self.triples[j], j == 0)

    def fields(self, j):
        """Party j's five base64 texts per object."""
        five = list(self.pre[j][:3]) + list(self.wu(j))
        return [[base64.b64encode(x[a:b].tobytes()) for x in five] for a, b in map(self.obj, range(len(self.counts)))]

    def begin(self, ctx, j, **kw):
        return ctx.parties_begin(self.shares[j], self.stride, self.masks[j], self.triples[j], self.woff, self.n, **kw)


_CASES = {}


def case(F, n, counts, stride=32, zero_objects=()):
    key = (n, tuple(counts), stride, tuple(zero_objects))
    if key not in _CASES:
        _CASES[key] = Case(F, n, counts, stride, zero_objects)
    return _CASES[key]


def run_party(ctx, c, j, partner_texts=None, b64=True):
    """Party j's whole session from host buffers; partner_texts[k] overrides
    party k's K texts.  -> (session results dict)."""
    s = c.begin(ctx, j)
    out = {"yrv": (s.y, s.r, s.v), "texts": s.texts(), "bad": {}}
    for slot, k in enumerate([k for k in range(c.n) if k != j], start=1):
        ts = (partner_texts or {}).get(k) or c.texts(k)
        out["bad"][k] = s.partner(slot, ts, status=True)
    if b64:
        fields, rej = s.finish_b64(j == 0)
        out["fields"], out["rejected"] = s.split_fields(fields), rej
    else:
        out["wu"] = s.finish(j == 0)
    s.close()
    return out


# 64 words = one 128-pair tile exactly, 65 straddles into a second, 700 gives ~15 spans (windows across 2-3 spans)
@pytest.mark.parametrize("n,counts,stride", [(3, [1, 0, 64, 65, 700, 129], 32), (2, [1, 0, 64, 65, 700, 129], 16),
                                              (1, [1, 0, 64, 65, 700, 129], 32), (16, [3, 130], 32)])
def test_sizes_against_the_tiles(ctx, F, n, counts, stride):
    c = case(F, n, counts, stride)
    for j in range(n):
        got = run_party(ctx, c, j, b64=(j % 2 == 0))
        for g, w in zip(got["yrv"], c.pre[j][:3]):
            assert np.array_equal(g, w)
        assert got["texts"] == c.texts(j), j
        for k, (bad, st) in got["bad"].items():
            assert st == OK and (bad == -1).all(), (j, k, bad)
        if "fields" in got:
            assert got["fields"] == c.fields(j) and not got["rejected"].any(), j
        else:
            ow, ou = c.wu(j)
            assert np.array_equal(got["wu"][0], ow) and np.array_equal(got["wu"][1], ou), j


def test_equals_the_single_session_per_object(ctx, F):
    c = case(F, 3, [1, 0, 64, 65, 700, 129])
    got = run_party(ctx, c, 1)
    texts = [c.texts(k) for k in range(3)]
    for o in range(len(c.counts)):
        a, b = c.obj(o)
        s = ctx.party_begin(c.shares[1][a:b], 32, c.masks[1][2 * a:2 * b], c.triples[1][2 * a:2 * b], 3)
        assert s.text() == got["texts"][o], o
        s.partner(1, texts[0][o])
        s.partner(2, texts[2][o])
        assert s.finish_b64(False) == got["fields"][o], o
        s.close()


def reorder_text(t: bytes) -> bytes:
    return re.sub(rb'\{"a":(-?\d+),"b":(-?\d+)\}', rb'{"b":\2,"a":\1}', t)


def test_mixed_forms_in_one_call(ctx, F):
    """The 1200-word object's diffs are all 0: {"a":0,"b":0} runs hold more than
    528 values per span, so it falls back to pair order between two objects in
    span form.  Then one object's partner text with whitespace and "b","a"
    order (pair order by the general grammar) beside compact neighbours."""
    c = case(F, 3, [700, 1200, 65], zero_objects=(1,))
    assert not c.pre[0][3][2 * 700:2 * 1900].any()
    assert c.texts(1)[1].startswith(b'[{"a":0,"b":0},{"a":0,"b":0}')
    for j in range(3):
        got = run_party(ctx, c, j)
        assert got["texts"] == c.texts(j)
        assert all(st == OK for _, st in got["bad"].values())
        assert got["fields"] == c.fields(j) and not got["rejected"].any(), j
    c2 = case(F, 3, [700, 300, 65])
    t1 = c2.texts(1)
    spaced = reorder_text(t1[1]).replace(b',"a"', b', "a"').replace(b"},{", b"},\n{")
    assert len(spaced) <= 8192 * ((92 * 600 + 2 + 8191) // 8192)
    got = run_party(ctx, c2, 0, partner_texts={1: [t1[0], spaced, t1[2]], 2: [reorder_text(t) for t in c2.texts(2)]})
    assert all(st == OK for _, st in got["bad"].values())
    assert got["fields"] == c2.fields(0) and not got["rejected"].any()


def sized_triples(c, o, length):
    """Edit party 1's tuples so that its text of object o is exactly `length`
    characters, by the digit counts of the diffs (the idea of the exchange
    batch suite's sized texts: 12 characters of frame per pair plus the
    digits, every fifth value negative).  K_ODO_PRE opens d = fromGfp(x) -
    fromGfp(a) with x the share / mask word and a the triple's factor: x becomes
    toGfp(p / 2 + w) and a = toGfp(p / 2 + w - d)."""
    a0, b0 = c.obj(o)
    npairs = 2 * (b0 - a0)
    budget = length - 1 - 12 * npairs
    nsign = (2 * npairs + 4) // 5
    base, extra = divmod(budget - nsign, 2 * npairs)
    assert 1 <= base and base + 1 <= 37

    def gfp(z):
        return np.frombuffer((z * R % P).to_bytes(16, "little"), np.uint8)

    t, sh, mk = c.triples[1], c.shares[1], c.masks[1]
    for w in range(a0, b0):
        sh[w, 0:16] = gfp(P // 2 + w)
        mk[2 * w, 0:16] = gfp(P // 2 + w)
        mk[2 * w + 1, 0:16] = gfp(P // 2 + w)
    for i in range(2 * npairs):
        nd = base + (1 if i < extra else 0)
        v = (i % 9) + 1 if nd == 1 else 10 ** (nd - 1) + (i * 7919) % (10 ** (nd - 1))
        if i % 5 == 0:
            v = -v
        k = 2 * a0 + i // 2
        t[k, 32 * (i % 2):32 * (i % 2) + 16] = gfp(P // 2 + k // 2 - v)


@pytest.mark.parametrize("length", [8191, 8192, 8193])
def test_text_length_edges(ctx, F, length):
    """One partner object's text is exactly 8191 / 8192 / 8193 characters
    (the second span is missing, empty of values, or holds one ']'), beside
    ordinary objects."""
    words = 51  # 204 values: 12 * 102 + 1 frame characters, the rest digits and signs
    key = ("edge", length)
    if key not in _CASES:
        def edit(c):
            sized_triples(c, 1, length)
        _CASES[key] = Case(F, 2, [130, words, 7], edit=edit)
    c = _CASES[key]
    assert len(c.texts(1)[1]) == length
    for j in range(2):
        got = run_party(ctx, c, j)
        assert got["texts"] == c.texts(j)
        assert all(st == OK and (bad == -1).all() for bad, st in got["bad"].values())
        assert got["fields"] == c.fields(j), j


def faults(text, pairs):
    at = len(text) // 2
    while not chr(text[at]).isdigit():
        at += 1
    return {
        "poked": text[:at] + b"x" + text[at + 1:],
        "unclosed": text[:-1],
        "short": (text[: text.rindex(b",{")] + b"]") if pairs > 1 else b"[]",
        "empty": b"",
    }


@pytest.mark.parametrize("which", [0, 2, 4])
def test_one_faulty_object_moves_only_itself(ctx, F, which):
    c = case(F, 3, [40, 65, 300, 9, 129])
    good = c.texts(1)
    want = c.fields(0)
    for name, bad_text in faults(good[which], 2 * c.counts[which]).items():
        ts = list(good)
        ts[which] = bad_text
        s = c.begin(ctx, 0, want_yrv=False)
        bad, st = s.partner(1, ts, status=True)
        import amphora_amd as A
        message = A._lib.lib.amph_last_error().decode()
        # the verdict of the single decode on that text alone
        try:
            ctx.exchange_decode(bad_text, 2 * c.counts[which])
            single = -1
        except ValueError as e:
            m = re.search(r"offset (\d+)", str(e))
            single = int(m.group(1)) if m else len(bad_text)
        assert bad[which] == single and single >= 0, (name, bad, single)
        assert (np.delete(bad, which) == -1).all(), (name, bad)
        assert st == (E_LEN if single == len(bad_text) else E_PARAM), (name, st)
        assert "object %d" % which in message, (name, message)
        s.partner(2, c.texts(2))
        fields, rej = s.finish_b64(True)
        got = s.split_fields(fields)
        assert list(rej) == [int(o == which) for o in range(5)], name
        for o in range(5):
            if o == which:
                assert all(f[:4] == b"!!!!" for f in got[o]), name
            else:
                assert got[o] == want[o], (name, o)
        s.close()
    # after a reset and a clean resubmission everything verifies
    ts = list(good)
    ts[which] = faults(good[which], 2 * c.counts[which])["poked"]
    s = c.begin(ctx, 0, want_yrv=False)
    assert s.partner(1, ts, status=True)[1] == E_PARAM
    s.reset_partner(1)
    assert (s.partner(1, good) == -1).all()
    s.partner(2, c.texts(2))
    fields, rej = s.finish_b64(True)
    assert s.split_fields(fields) == want and not rej.any()
    s.close()


def test_device_mode(ctx, F):
    """Three parties on one side stream: each party's text_dev buffers go
    straight into the others' partner_dev, the verdicts are device arrays the
    caller overwrites right after the call, the fields are read back once."""
    import torch
    c = case(F, 3, [1, 0, 64, 65, 700, 129])
    K = len(c.counts)
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()  # noqa: E731
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        inputs = [(dev(c.shares[j]), dev(c.masks[j]), dev(c.triples[j])) for j in range(3)]
        for poisoned in (None, 4):
            sessions = [ctx.parties_begin_dev(inputs[j][0], 32, inputs[j][1], inputs[j][2], c.woff, 3, want_yrv=True)
                        for j in range(3)]
            texts = [s.text_dev() for s in sessions]
            if poisoned is not None:  # party 1's text of one object gets a byte poked, in a copy of its buffer
                t = texts[1][0].clone()
                t[int(sessions[1].text_offsets[poisoned]) + 40] = ord("x")
                texts[1] = (t, texts[1][1], texts[1][2])
            verdicts, fields = [], []
            for j, s in enumerate(sessions):
                for slot, k in enumerate([k for k in range(3) if k != j], start=1):
                    bad = s.partner(slot, texts[k][0], texts[k][2])
                    verdicts.append((j, k, bad.clone()))
                    bad.fill_(0)  # the caller's words are free once the stream has passed the call
                fields.append(s.finish_b64(j == 0))
            side.synchronize()
            for j, k, v in verdicts:
                v = v.cpu().numpy()
                if poisoned is not None and k == 1:
                    assert 0 <= v[poisoned] <= 40 and (np.delete(v, poisoned) == NO_FAILURE).all()
                else:
                    assert (v == NO_FAILURE).all(), (j, k, v)
            for j, s in enumerate(sessions):
                assert sessions[j].texts() == c.texts(j)
                for g, w in zip((s.y, s.r, s.v), c.pre[j][:3]):
                    assert np.array_equal(g.cpu().numpy(), w)
                got = s.split_fields([f.cpu().numpy() for f in fields[j]])
                want = c.fields(j)
                for o in range(K):
                    if poisoned == o and j != 1:
                        assert all(f[:4] == b"!!!!" for f in got[o])
                    else:
                        assert got[o] == want[o], (j, o)
            for s in sessions:
                s.close()


def test_launch_count_does_not_depend_on_k_and_the_pool_serves_the_second_session(ctx, F):
    import torch

    def launches(counts):
        c = case(F, 3, counts)
        before = ctx.stats()["kernel_launches"]
        s = c.begin(ctx, 0, want_yrv=False)
        s.partner(1, c.texts(1))
        s.partner(2, c.texts(2))
        s.finish_b64(True)
        after = ctx.stats()["kernel_launches"]
        s.close()
        return after - before

    assert launches([300]) == launches([25] * 12)
    c = case(F, 3, [25] * 12)
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()  # noqa: E731
    d = (dev(c.shares[0]), dev(c.masks[0]), dev(c.triples[0]))
    ctx.parties_begin_dev(d[0], 32, d[1], d[2], c.woff, 3).close()
    pooled = ctx.stats()
    s = ctx.parties_begin_dev(d[0], 32, d[1], d[2], c.woff, 3)
    during = ctx.stats()
    s.close()
    after = ctx.stats()
    # the second session took its buffer from the pool and put the same one back: nothing was allocated
    assert during["pool_buffers"] == pooled["pool_buffers"] - 1 and during["pool_bytes"] < pooled["pool_bytes"]
    assert (after["pool_buffers"], after["pool_bytes"]) == (pooled["pool_buffers"], pooled["pool_bytes"])


def test_session_errors_return_before_any_gpu_work(ctx, F):
    """The checks that need a session: a host call on a device session and the
    reverse, an unfilled slot at finish, a second finish, a slot filled twice."""
    import torch
    import amphora_amd as A
    c = case(F, 3, [40, 65, 300, 9, 129])
    s = c.begin(ctx, 0, want_yrv=False)
    before = ctx.stats()["kernel_launches"]
    with pytest.raises(A.AmphoraNativeError, match="partner slot 1's interimValues texts are missing"):
        s.finish(True)
    for slot in (0, 3, -1):
        with pytest.raises(A.AmphoraNativeError, match=r"partner slot must be in \[1, 2\]"):
            s.partner(slot, c.texts(1))
    import ctypes
    lib, arr = A._lib.lib, (ctypes.c_void_p * 5)()
    assert lib.amph_parties_finish_b64_dev(s._h, 1, arr, None) == E_PARAM
    assert "takes the host calls" in lib.amph_last_error().decode()
    v = np.zeros(8, np.uint64)
    assert lib.amph_parties_text_dev(s._h, arr, arr, arr) == E_PARAM
    assert "takes the host calls" in lib.amph_last_error().decode()
    long = c.texts(1)
    long[3] = b" " * (SPAN + 1)
    with pytest.raises(A.AmphoraNativeError, match="object 3: a text of 8193 characters runs past its slot"):
        s.partner(1, long)
    assert ctx.stats()["kernel_launches"] == before
    s.partner(1, c.texts(1))
    with pytest.raises(A.AmphoraNativeError, match="slot 1 already holds its texts"):
        s.partner(1, c.texts(1))
    with pytest.raises(A.AmphoraNativeError, match="partner slot 2's interimValues texts are missing"):
        s.finish_b64(True)
    s.partner(2, c.texts(2))
    w, u = s.finish(True)
    assert np.array_equal(w, c.wu(0)[0]) and np.array_equal(u, c.wu(0)[1])
    with pytest.raises(A.AmphoraNativeError, match="already finished"):
        s.finish(True)
    s.close()
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()  # noqa: E731
    d = ctx.parties_begin_dev(dev(c.shares[0]), 32, dev(c.masks[0]), dev(c.triples[0]), c.woff, 3)
    for st in (lib.amph_parties_partner(d._h, 1, v.ctypes.data, v.ctypes.data, v.ctypes.data),
               lib.amph_parties_text_lens(d._h, v.ctypes.data), lib.amph_parties_text(d._h, 0, v.ctypes.data, 0),
               lib.amph_parties_finish(d._h, 1, v.ctypes.data, v.ctypes.data),
               lib.amph_parties_finish_b64(d._h, 1, arr, None)):
        assert st == E_PARAM and "takes the *_dev calls" in lib.amph_last_error().decode()
    with pytest.raises(A.AmphoraNativeError, match="finishes with finish_b64"):
        d.finish(True)
    d.close()


class Cluster:
    """n loopback parties over the fake dealer, with K secrets uploaded."""

    def __init__(self, n, sizes, seed, fmt):
        import random
        from concurrent.futures import ThreadPoolExecutor
        import amphora_amd as A
        from amphora_amd.loopback import AmphoraParty, ExchangeHub, LoopbackAmphoraClient
        from tests.loopback_dealer import FakeCastor
        rng = random.Random(seed)
        keys = [rng.randrange(P) for _ in range(n)]
        self.castor = FakeCastor(P, R, RINV, keys, seed)
        self.hub = ExchangeHub(n, timeout_s=20)
        self.parties = [AmphoraParty(j, P, R, RINV, keys[j], self.castor, self.hub, exchange_format=fmt)
                        for j in range(n)]
        self.client = LoopbackAmphoraClient(self.parties, P, R, RINV)
        self.sids = [self.client.create_secret(A.Secret.of([("n", str(o))], [rng.randrange(P) for _ in range(W)]))
                     for o, W in enumerate(sizes)]
        self.pool = ThreadPoolExecutor(max_workers=n)

    def shares(self, p):
        """The uploaded secrets' shares and one empty request."""
        import amphora_amd as A
        got = [p.secrets[s] for s in self.sids]
        return got[:2] + [A.SecretShare(uuid.UUID(int=77), b"", [])] + got[2:]

    def all(self, fn):
        return [f.result() for f in [self.pool.submit(fn, p) for p in self.parties]]

    def close(self):
        self.pool.shutdown()
        self.client.close()


def test_service_mirror_runs_the_requests_as_one_batch_session():
    """exchange_format="session_batch", three parties, K = 4 with an empty
    request: the ODOs of exchange_format="objects"; then, on party 0 alone, one
    request's tuple download raises and another's partner body carries a wrong
    operation id: each gets the single function's exception, the rest their
    ODOs."""
    import amphora_amd as A
    from amphora_amd import service, wire
    sizes = [5, 130, 64]
    rids = [uuid.UUID(int=999000 + o) for o in range(4)]
    ref = Cluster(3, sizes, 53, "objects")
    try:
        want = ref.all(lambda p: p.odo_service.compute_output_delivery_objects(ref.shares(p), rids))
    finally:
        ref.close()
    c = Cluster(3, sizes, 53, "session_batch")
    try:
        batch = c.all(lambda p: p.odo_service.compute_output_delivery_objects(c.shares(p), rids))
        for j in range(3):
            for o in range(4):
                assert isinstance(batch[j][o], A.OutputDeliveryObject), (j, o, batch[j][o])
                assert list(batch[j][o].fields()) == list(want[j][o].fields()), (j, o)
        one = c.all(lambda p: p.odo_service.compute_output_delivery_object(c.shares(p)[1], rids[1]))  # a batch of one
        assert [list(x.fields()) for x in one] == [list(want[j][1].fields()) for j in range(3)]
        # party 0 alone (the hub holds the partners' bodies of every operation)
        p0 = c.parties[0]
        svc = p0.odo_service
        exchange, tuples = svc._exchange, svc._tuples
        shares = c.shares(p0)
        bad_op = service.name_uuid_from_bytes(("%s_%d" % (rids[3], 2 * sizes[2])).encode())
        other = uuid.UUID(int=12345)

        def renaming_exchange(body):
            partners = [bytes(b) for b in exchange(body)]
            if wire.exchange_header(bytes(body))[0] == bad_op:
                partners[1] = partners[1].replace(str(bad_op).encode(), str(other).encode(), 1)
            return partners

        def failing_tuples(request_id, tuple_type, count):
            if request_id == rids[0]:
                raise RuntimeError("castor is down")
            return tuples(request_id, tuple_type, count)
        svc._exchange, svc._tuples = renaming_exchange, failing_tuples
        try:
            got = svc.compute_output_delivery_objects(shares, rids)
            singles = []
            for o in (0, 3):
                with pytest.raises(A.AmphoraServiceException) as single:
                    svc.compute_output_delivery_object(shares[o], rids[o])
                singles.append(single.value)
        finally:
            svc._exchange, svc._tuples = exchange, tuples
        assert type(got[0]) is A.AmphoraServiceException and str(got[0]) == str(singles[0])
        assert str(got[0]) == "Failed to retrieve the required Tuples form Castor"
        assert type(got[3]) is A.AmphoraServiceException and str(got[3]) == str(singles[1])
        assert str(got[3]) == "Failed to open values for operation #%s" % bad_op
        assert str(got[3].__cause__) == "operation id %s != %s" % (other, bad_op)
        for o in (1, 2):
            assert list(got[o].fields()) == list(want[0][o].fields()), o
    finally:
        c.close()
