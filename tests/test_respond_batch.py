"""Many Output Delivery responses' base64 fields per launch, on the GPU
(include/amphora_respond_batch.h: amph_odo_fields_b64_packed / _batch, kernel
k_odo_b64_seg).

Expected texts come from Python's base64 on each object's own bytes of each
field; every text is also compared with the library's single
amph_base64_encode.  192 words are one workgroup's tile: the size list holds
the three paddings (1, 2, 3 words), both edges of the tile, two and three
tiles, an object of exactly whole tiles and empty objects first, in the middle
and last.  The round trips take honest n-party ODOs and their secrets from the
C restatement oracle/coracle."""
import base64
import ctypes as C
import functools
import json
import random
import subprocess
import sys
import uuid
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import amphora_oracle as O
from oracle import coracle
from tests import extent_cases as X
from tests import field_cases as FC
from tests.test_respond_batch_cpu import BROKEN_DEVICE_TABLES, ROOT

pytestmark = pytest.mark.gpu

P, R, RINV = O.TEST_PRIME, O.TEST_R, O.TEST_RINV
NF = 0x7F7F7F7F7F7F7F7F
OK = 0
F_DEVICE = 1
SIZES = [0, 1, 2, 3, 191, 192, 193, 0, 385, 576, 0]
K, T = len(SIZES), sum(SIZES)
WOFF = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.uint64)
MODES = ["host_packed", "host_batch", "device_packed"]
REJECTED = (2, 5)  # 2 words and one whole tile, clean objects between and around


def nchars_of(words):
    return 4 * ((16 * words + 2) // 3)


def slots(gap):
    """text_offsets with `gap` unused characters after every 16-aligned slot, and the buffers' length."""
    toff, at = [], 0
    for W in SIZES:
        toff.append(at)
        at += -(-nchars_of(W) // 16) * 16 + gap
    return np.array(toff, np.uint64), at


@functools.lru_cache(maxsize=None)
def _ctx():
    import amphora_amd as A
    return A.Context(P, R, RINV)


@functools.lru_cache(maxsize=None)
def fields():
    """Five (T, 16) arrays of random bytes with runs of 0x00 and 0xFF, and the
    expected text of every object and field, computed once."""
    rng = np.random.default_rng(20260)
    f = rng.integers(0, 256, (5, T, 16), dtype=np.uint8)
    f[0, 3:40] = 0x00       # across the 1-, 2-, 3-word objects into the 191-word one
    f[1, 190:200] = 0xFF    # across two objects' border
    f[2, 389:391] = 0x00    # the words either side of the whole-tile object's end
    f[3, :7] = 0xFF
    f[4, 967:1543:5] = 0xFF
    f[4, 1542] = 0x00       # the last word
    f.setflags(write=False)
    want = [[base64.b64encode(f[k, int(WOFF[o]):int(WOFF[o + 1])].tobytes()) for k in range(5)] for o in range(K)]
    assert [len(w[0]) for w in want] == [nchars_of(W) for W in SIZES]
    assert want[1][0].endswith(b"==") and want[2][0].endswith(b"=") and not want[2][0].endswith(b"==") \
        and not want[3][0].endswith(b"=")
    return f, want


def _dev(x):
    import torch
    x = np.array(x, copy=True)
    return torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).cuda()


def _host(v):
    import torch
    torch.cuda.synchronize()
    return v.cpu().numpy()


def run(mode, gap=0, reject=None):
    """-> (texts[o][k], the five whole buffers or None, their fill before the call, text_offsets)."""
    f, _ = fields()
    ctx = _ctx()
    if mode == "host_batch":
        objs = [[np.ascontiguousarray(f[k, int(WOFF[o]):int(WOFF[o + 1])]) for k in range(5)] for o in range(K)]
        rj = None if reject is None else [0 if o in reject else -1 for o in range(K)]
        return ctx.odo_fields_b64_batch(objs, reject=rj), None, None, None
    toff, nchars = slots(gap)
    fill = X.band_pattern(7, nchars + 64)  # 64 characters behind the last slot as well
    if mode == "host_packed":
        out = [fill.copy() for _ in range(5)]
        rj = None if reject is None else np.array([3 if o in reject else -1 for o in range(K)], np.int64)
        bufs, to = ctx.odo_fields_b64_packed([np.ascontiguousarray(f[k]) for k in range(5)], WOFF, toff, out=out,
                                             reject=rj)
    else:
        out = [_dev(fill) for _ in range(5)]
        rj = None if reject is None else _dev(np.array([9 if o in reject else NF for o in range(K)], np.int64))
        bufs, to = ctx.odo_fields_b64_packed([_dev(f[k]) for k in range(5)], _dev(WOFF), _dev(toff), out=out,
                                             reject=rj)
        bufs, to = [_host(b) for b in bufs], _host(to)
    assert [int(x) for x in to] == [int(x) for x in toff]
    texts = [[bufs[k][int(toff[o]):int(toff[o]) + nchars_of(SIZES[o])].tobytes() for k in range(5)] for o in range(K)]
    return texts, bufs, fill, toff


def check_texts(texts, reject=()):
    _, want = fields()
    for o in range(K):
        for k in range(5):
            if o in reject and SIZES[o]:
                assert texts[o][k][:4] == b"!!!!" and len(texts[o][k]) == len(want[o][k]), (o, k)
            else:
                assert texts[o][k] == want[o][k], (o, k)


def check_gaps(bufs, fill, toff):
    keep = np.ones(fill.size, bool)
    for o in range(K):
        keep[int(toff[o]):int(toff[o]) + nchars_of(SIZES[o])] = False
    for k in range(5):
        d = np.nonzero((bufs[k] != fill) & keep)[0]
        assert d.size == 0, "field %d: character %d outside every text changed" % (k, int(d[0]))


# ---- 1. parity and layout -----------------------------------------------------------
@pytest.mark.parametrize("gap", [0, 16, 48])
@pytest.mark.parametrize("mode", ["host_packed", "device_packed"])
def test_packed_parity_and_untouched_gaps(mode, gap):
    texts, bufs, fill, toff = run(mode, gap)
    check_texts(texts)
    check_gaps(bufs, fill, toff)


def test_batch_parity():
    texts, _, _, _ = run("host_batch")
    check_texts(texts)


def test_default_layout_is_the_dense_one():
    import amphora_amd as A
    f, want = fields()
    bufs, to = _ctx().odo_fields_b64_packed([_dev(f[k]) for k in range(5)], WOFF)
    dense, end = slots(0)
    assert [int(x) for x in _host(to)] == [int(x) for x in dense] and bufs[0].numel() == end
    strides = [int(b) - int(a) for a, b in zip(dense, list(dense[1:]) + [end])]
    assert [A._lib.wire_slot_chars(W) for W in SIZES] == strides
    got = _host(bufs[3])
    assert all(got[int(dense[o]):int(dense[o]) + len(want[o][3])].tobytes() == want[o][3] for o in range(K))


def test_expected_texts_equal_the_single_encode():
    f, want = fields()
    ctx = _ctx()
    for o in range(K):
        for k in range(5):
            assert ctx.base64_encode(f[k, int(WOFF[o]):int(WOFF[o + 1])].tobytes()) == want[o][k], (o, k)


# ---- 2. reject ------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_rejected_objects_are_marked_and_the_rest_is_exact(mode):
    texts, bufs, fill, toff = run(mode, 16, reject=REJECTED)
    check_texts(texts, reject=REJECTED)
    if bufs is not None:
        check_gaps(bufs, fill, toff)


@pytest.mark.parametrize("mode", MODES)
def test_rejecting_an_empty_object_writes_nothing(mode):
    texts, bufs, fill, toff = run(mode, 16, reject=(0, 7, 10))
    check_texts(texts)
    if bufs is not None:
        check_gaps(bufs, fill, toff)


# ---- 3. device round trip -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def honest(n):
    F = coracle.Field(P, R, RINV, threads=4)
    odos, _ = F.synth_odos(seed=8100 + n, n=n, W=T, noncanon_permille=100)
    odos = [tuple(np.ascontiguousarray(f) for f in o) for o in odos]
    y, ff = F.recombine_verify(odos)
    assert ff == -1
    return odos, y


def round_trip(odos, reject0=None):
    """Each party's five buffers from its own call, then the client's packed verify on them."""
    ctx = _ctx()
    dwo = _dev(WOFF)
    texts, dto = [], None
    for j, od in enumerate(odos):  # the default layout: dense slots, the same table from every call
        bufs, dto = ctx.odo_fields_b64_packed([_dev(f) for f in od], dwo, reject=reject0 if j == 0 else None)
        texts.append(tuple(bufs))
    sec, ff, bad = ctx.recombine_verify_b64_packed(texts, dwo, dto)
    return _host(sec), [int(x) for x in _host(ff)], [int(x) for x in _host(bad)]


@pytest.mark.parametrize("n", [2, 3])
def test_device_round_trip_to_the_secrets(n):
    odos, y = honest(n)
    sec, ff, bad = round_trip(odos)
    assert ff == [NF] * K and bad == [NF] * K
    assert np.array_equal(sec, y)


@pytest.mark.parametrize("n", [2, 3])
def test_device_round_trip_finds_a_planted_fault_in_its_object(n):
    odos, y = honest(n)
    o, local = 8, 200  # the 385-word object, its second tile
    sec, ff, bad = round_trip(FC.with_fault(odos, int(WOFF[o]) + local))
    assert bad == [NF] * K and ff == [local if i == o else NF for i in range(K)]
    keep = np.ones(T, bool)
    keep[int(WOFF[o]):int(WOFF[o + 1])] = False
    assert np.array_equal(sec[keep], y[keep])


@pytest.mark.parametrize("n", [2, 3])
def test_device_round_trip_sees_a_rejected_object_as_bad_text(n):
    odos, y = honest(n)
    o = 6  # 193 words
    rj = _dev(np.array([17 if i == o else NF for i in range(K)], np.int64))
    sec, ff, bad = round_trip(odos, reject0=rj)
    assert bad == [0 if i == o else NF for i in range(K)]
    assert [ff[i] for i in range(K) if i != o] == [NF] * (K - 1)
    keep = np.ones(T, bool)
    keep[int(WOFF[o]):int(WOFF[o + 1])] = False
    assert np.array_equal(sec[keep], y[keep])


# ---- 4. guard bands --------------------------------------------------------------------
def plans(device):
    """The test's own plan table: slots with 16- and 48-character gaps, with and without reject."""
    f, want = fields()
    for gap in (16, 48):
        for with_reject in (False, True):
            toff, nchars = slots(gap)
            rej = REJECTED if with_reject else ()
            ins = [X.Arr("f%d" % k, X.WORD, data=f[k]) for k in range(5)]
            ins += [X.Arr("woff", X.OFFS, data=WOFF), X.Arr("toff", X.OFFS, data=toff)]
            if with_reject:
                none = NF if device else -1
                ins.append(X.Arr("reject", X.VERDICT, data=np.array([5 if o in rej else none for o in range(K)],
                                                                    np.int64)))
            outs = [X.Arr("o%d" % k, X.B64, n=nchars) for k in range(5)]
            before = {}

            def call(L, h, p, fl, s, nchars=nchars, with_reject=with_reject):
                import amphora_amd as A
                odo = A._lib._AmphOdo(*[p["f%d" % k] for k in range(5)], 16 * T)
                ob = A._lib._AmphOdoB64Out(*[p["o%d" % k] for k in range(5)], nchars)
                return L.amph_odo_fields_b64_packed(h, C.byref(odo), p["woff"], p["toff"], K, C.byref(ob),
                                                    p["reject"] if with_reject else None, fl, s)

            def check(whole, toff=toff, rej=rej, before=before):
                for k in range(5):
                    pay = np.frombuffer(whole["o%d" % k], np.uint8)
                    keep = np.ones(pay.size, bool)
                    for o in range(K):
                        a, nc = int(toff[o]), nchars_of(SIZES[o])
                        keep[a:a + nc] = False
                        got = pay[a:a + nc].tobytes()
                        if o in rej:
                            assert got[:4] == b"!!!!", (k, o)
                        else:
                            assert got == want[o][k], (k, o)
                    d = np.nonzero((pay != before["o%d" % k]) & keep)[0]
                    assert d.size == 0, "o%d: character %d outside every text changed" % (k, int(d[0]))

            yield X.Plan("odo_fields_b64_packed gap=%d reject=%s" % (gap, with_reject), ins, outs, call,
                         check=check), before


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_guard_bands_both_surrounds(device):
    import torch
    import amphora_amd as A
    L, ctx = A._lib.lib, _ctx()
    flags = F_DEVICE if device else 0
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream) if device else None
    ran = 0
    for plan, before in plans(device):
        def invoke(ins, outs, plan=plan, before=before):
            for name, g in outs.items():  # the pattern the payload holds before the call
                before[name] = g.before[g.lo:g.lo + g.n].copy()
            p = {k: g.ptr for k, g in list(ins.items()) + list(outs.items())}
            return plan.call(L, ctx._h, p, flags, stream)
        X.run_plan(plan, device, invoke, torch.cuda.synchronize)
        ran += 1
    assert ran == 4


# ---- 5. broken device tables -----------------------------------------------------------
@pytest.mark.parametrize("name", sorted(BROKEN_DEVICE_TABLES))
def test_broken_device_tables_stay_inside_the_buffers(name):
    """AMPH_F_DEVICE leaves the tables to the caller; whatever they hold, nothing
    outside the five arrays' T words is read and nothing outside the five
    buffers' nchars characters written.  The same table first passes the host
    geometry program (tests/test_respond_batch_cpu.py), which states every
    tile's ranges; only the bounds are asserted here, nothing about values."""
    import torch
    import amphora_amd as A
    sys.path.insert(0, ROOT + "/tools")
    import build_native
    Tn, nchars, woff, toff = BROKEN_DEVICE_TABLES[name]
    args = [str(x) for x in [Tn, nchars, len(toff)] + woff + toff]
    r = subprocess.run([build_native.build_respondtiles_test(), "tables"] + args, capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "inside", r.stdout + r.stderr
    Kn = len(toff)
    rng = np.random.default_rng(5)
    main = X.Arena(True)
    g_in = [main.add("f%d" % k, X.WORD, data=rng.integers(0, 256, 16 * Tn, dtype=np.uint8), fill="hostile")
            for k in range(5)]
    g_w = main.add("woff", X.OFFS, data=np.array(woff, np.uint64), fill="zeros")
    g_t = main.add("toff", X.OFFS, data=np.array(toff, np.uint64), fill="zeros")
    g_r = main.add("reject", X.VERDICT, data=np.zeros(Kn, np.int64), fill="zeros")  # every object rejected
    g_out = [main.add("o%d" % k, X.B64, n=nchars) for k in range(5)]
    main.commit()
    odo = A._lib._AmphOdo(*[g.ptr for g in g_in], 16 * Tn)
    ob = A._lib._AmphOdoB64Out(*[g.ptr for g in g_out], nchars)
    st = A._lib.lib.amph_odo_fields_b64_packed(_ctx()._h, C.byref(odo), g_w.ptr, g_t.ptr, Kn, C.byref(ob), g_r.ptr,
                                               F_DEVICE, None)
    torch.cuda.synchronize()
    main.fetch()
    assert st == OK
    for g in main.items:
        (g.check_untouched if g in g_out else g.check_unchanged)()


# ---- 6. copies and launches --------------------------------------------------------------
def test_copies_and_launches_do_not_grow_with_k():
    import amphora_amd as A
    ctx = A.Context(P, R, RINV)
    f, want = fields()
    c0, l0 = ctx.respond_batch_copies(), ctx.stats()["kernel_launches"]
    objs = [[np.ascontiguousarray(f[k, int(WOFF[o]):int(WOFF[o + 1])]) for k in range(5)] for o in range(K)]
    assert ctx.odo_fields_b64_batch(objs) == want  # 1,543 words: the small-call arena
    assert (ctx.respond_batch_copies() - c0, ctx.stats()["kernel_launches"] - l0) == (0, 1)
    Tn = 12800
    assert Tn * 5 * (16 + 64 // 3) > (2 << 20)  # above the default AMPH_SMALL_BYTES: the staged path
    big = np.random.default_rng(77).integers(0, 256, (5, Tn, 16), dtype=np.uint8)
    deltas = []
    for Kn in (2, 64):
        W = Tn // Kn
        objs = [[np.ascontiguousarray(big[k, o * W:(o + 1) * W]) for k in range(5)] for o in range(Kn)]
        c0, l0 = ctx.respond_batch_copies(), ctx.stats()["kernel_launches"]
        texts = ctx.odo_fields_b64_batch(objs)
        deltas.append((ctx.respond_batch_copies() - c0, ctx.stats()["kernel_launches"] - l0))
        assert texts == [[base64.b64encode(big[k, o * W:(o + 1) * W].tobytes()) for k in range(5)]
                         for o in range(Kn)]
    assert deltas == [(2, 1), (2, 1)]


# ---- 7. mirrors -------------------------------------------------------------------------
def _odo_of(o):
    import amphora_amd as A
    f, _ = fields()
    return A.OutputDeliveryObject(*[f[k, int(WOFF[o]):int(WOFF[o + 1])].tobytes() for k in range(5)])


def test_wire_mirrors_equal_the_single_functions_entry_by_entry():
    from amphora_amd import wire
    ctx = _ctx()
    objs = [1, 3, 4, 5, 8]
    odos = [_odo_of(o) for o in objs]
    sids = [uuid.UUID(int=9000 + o) for o in objs]
    tags = [[("k", "v")] if o % 2 else [] for o in objs]
    for pretty in (True, False):
        got = wire.vss_bodies_to_json(ctx, sids, tags, odos, pretty=pretty)
        assert got == [wire.vss_to_json(ctx, s, t, od, pretty=pretty) for s, t, od in zip(sids, tags, odos)]
    assert wire.odo_bodies_to_json(ctx, odos) == [wire.odo_to_json(ctx, od) for od in odos]
    _, want = fields()
    assert json.loads(wire.odo_bodies_to_json(ctx, odos)[2])["wShares"] == want[4][3].decode()
    assert wire.odo_bodies_to_json(ctx, []) == [] and wire.vss_bodies_to_json(ctx, [], [], []) == []


class Cluster:
    """Two loopback parties over the fake dealer, with K secrets uploaded."""

    def __init__(self, fmt, sizes, seed):
        import amphora_amd as A
        from amphora_amd.loopback import AmphoraParty, ExchangeHub, LoopbackAmphoraClient
        from tests.loopback_dealer import FakeCastor
        rng = random.Random(seed)
        keys = [rng.randrange(P) for _ in range(2)]
        self.castor = FakeCastor(P, R, RINV, keys, seed)
        self.hub = ExchangeHub(2, timeout_s=20)
        self.parties = [AmphoraParty(j, P, R, RINV, keys[j], self.castor, self.hub, exchange_format=fmt)
                        for j in range(2)]
        self.client = LoopbackAmphoraClient(self.parties, P, R, RINV)
        self.data = [[rng.randrange(P) for _ in range(W)] for W in sizes]
        self.sids = [self.client.create_secret(A.Secret.of([("n", str(o))], d)) for o, d in enumerate(self.data)]
        self.pool = ThreadPoolExecutor(max_workers=2)

    def both(self, fn):
        return [f.result() for f in [self.pool.submit(fn, p) for p in self.parties]]

    def close(self):
        self.pool.shutdown()
        self.client.close()


def _same_odo(a, b):
    return list(a.fields()) == list(b.fields())


@pytest.mark.parametrize("fmt", ["objects", "json"])
def test_service_mirror_is_bit_for_bit_the_single_function(fmt):
    import amphora_amd as A
    from amphora_amd import client, service, wire
    sizes = [1, 5, 192, 40, 3, 193]
    c = Cluster(fmt, sizes, seed=31 + len(fmt))
    try:
        rids = [uuid.UUID(int=555000 + o) for o in range(len(sizes))]
        before = [p.ctx.stats()["kernel_launches"] for p in c.parties]
        batch = c.both(lambda p: p.odo_service.compute_output_delivery_objects([p.secrets[s] for s in c.sids], rids))
        launches = [p.ctx.stats()["kernel_launches"] - b for p, b in zip(c.parties, before)]
        singles = [c.both(lambda p, o=o: p.odo_service.compute_output_delivery_object(p.secrets[c.sids[o]], rids[o]))
                   for o in range(len(sizes))]
        for j in range(2):
            for o in range(len(sizes)):
                assert isinstance(batch[j][o], A.OutputDeliveryObject) and _same_odo(batch[j][o], singles[o][j]), (j, o)
        if fmt == "objects":  # K_ODO_PRE and the open + K_ODO_POST once for all six requests, not six times
            assert [6 * n for n in launches] == [p.ctx.stats()["kernel_launches"] - b - n
                                                 for p, b, n in zip(c.parties, before, launches)]
        # through the response bodies and the client's batch verify back to the secrets
        bodies = [wire.vss_bodies_to_json(p.ctx, c.sids, [p.secrets[s].tags for s in c.sids], batch[j], pretty=False)
                  for j, p in enumerate(c.parties)]
        got = client.verify_vss_json_batch(c.client.util, [[bodies[0][o], bodies[1][o]] for o in range(len(sizes))])
        for o, g in enumerate(got):
            assert not isinstance(g, Exception), g
            assert g[0] == c.sids[o] and g[2] == c.data[o], o
        # request 1's tuple source raises, request 4's exchange raises: party 0 alone, the hub holds
        # party 1's diffs of every operation already
        p0 = c.parties[0]
        svc = p0.odo_service
        tuples, exchange = svc._tuples, svc._exchange
        bad_op = service.name_uuid_from_bytes(("%s_%d" % (rids[4], 2 * sizes[4])).encode())

        def failing_tuples(rid, ttype, count):
            if rid == rids[1]:
                raise RuntimeError("castor is down")
            return tuples(rid, ttype, count)

        def failing_exchange(xo):
            op = xo.operation_id if hasattr(xo, "operation_id") else wire.exchange_header(bytes(xo))[0]
            if op == bad_op:
                raise TimeoutError("no answer")
            return exchange(xo)

        svc._tuples, svc._exchange = failing_tuples, failing_exchange
        try:
            got = svc.compute_output_delivery_objects([p0.secrets[s] for s in c.sids], rids)
            for o in range(len(sizes)):
                try:
                    single = svc.compute_output_delivery_object(p0.secrets[c.sids[o]], rids[o])
                except A.AmphoraServiceException as e:
                    single = e
                if o in (1, 4):
                    assert isinstance(single, A.AmphoraServiceException)
                    assert type(got[o]) is type(single) and str(got[o]) == str(single), (o, got[o], single)
                else:
                    assert _same_odo(got[o], batch[0][o]) and _same_odo(got[o], single), o
            assert str(got[1]) == "Failed to retrieve the required Tuples form Castor"
            assert str(got[4]) == "Failed to open values for operation #%s" % bad_op
        finally:
            svc._tuples, svc._exchange = tuples, exchange
    finally:
        c.close()


def test_input_mask_mirror_is_bit_for_bit_the_single_function():
    import amphora_amd as A
    c = Cluster("json", [], seed=77)
    try:
        rids = [uuid.UUID(int=777000 + o) for o in range(4)]
        counts = [2, 193, 1, 64]
        batch = c.both(lambda p: p.odo_service.get_input_masks_as_output_delivery_objects(rids, counts))
        singles = [c.both(lambda p, o=o: p.odo_service.get_input_masks_as_output_delivery_object(rids[o], counts[o]))
                   for o in range(4)]
        for j in range(2):
            for o in range(4):
                odo, masks = batch[j][o]
                assert isinstance(odo, A.OutputDeliveryObject) and _same_odo(odo, singles[o][j][0]), (j, o)
                assert np.array_equal(masks, singles[o][j][1])
                assert len(odo.secret_shares) == 16 * counts[o]
    finally:
        c.close()
