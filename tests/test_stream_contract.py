"""Every device-mode call held to its stream (tests/stream_cases.py): the
inputs of a call arrive on a side stream behind a time-based gate, so at the
moment of the call the device holds zeros, and the outputs are copied back on
the same stream with no host synchronisation in between.

  S1 (order)    status, outputs, verdicts, bands and inputs equal the
                reference (P1-P3 of tests/extent_cases.py): every launch,
                memset and copy of the call is ordered on the caller's stream.
  S2 (no wait)  the call returned before its stream had passed the gate.

test_call_follows_its_stream runs both for every device entry of
extent_cases.CALLS (prime PIDS[0]; the smallest and largest size at the first
and last party count) and for the five device-mode calls of the batch headers.
The other tests run chains without a host synchronisation, two streams whose
execution order differs from the enqueue order on one context, two threads on
one context, and chains captured in a graph and replayed on rewritten inputs.
References: the C oracle, Python ints, base64, json -- never the library.
"""
import base64
import ctypes as C
import os
import re
import threading
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import extent_cases as X  # noqa: E402
from tests import field_cases as FC  # noqa: E402
from tests import stream_cases as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [c.id for c in S.device_calls()] + [name for name, _ in S.BATCH_CALLS]
F_ACCUMULATE = 2


class Env:
    def __init__(self):
        import torch
        assert torch.cuda.is_available()
        import amphora_amd as A
        self.torch, self.A, self.L = torch, A, A._lib.lib
        self.d = X.data(X.PIDS[0])
        self.ctx = self.context()
        self.gate = S.Gate()
        self.s1, self.s2 = torch.cuda.Stream(), torch.cuda.Stream()

    def context(self):
        pr = self.d.pr
        return self.A.Context(pr.p, pr.r, pr.rinv)

    def invoker(self, plan, stream, ctx=None):
        h, sp = (ctx or self.ctx)._h, C.c_void_p(stream.cuda_stream)
        assert sp.value, "a side stream, never the default one"

        def invoke(ins, outs):
            p = {k: g.ptr for k, g in list(ins.items()) + list(outs.items())}
            return plan.call(self.L, h, p, X.F_DEVICE, sp)
        return invoke

    def plans(self, ident):
        if ident in dict(S.BATCH_CALLS):
            return [S.batch_plan(ident)]
        return S.select(next(c for c in S.device_calls() if c.id == ident), self.d)

    def find(self, ident, label):
        call = next(c for c in S.device_calls() if c.id == ident)
        return next(p for p in call.gen(self.d) if p.label == label)


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    S._BATCH_PLANS.clear()


# ---- S1 and S2, call by call ---------------------------------------------------------------
@pytest.mark.parametrize("ident", IDS)
def test_call_follows_its_stream(env, ident):
    ran = 0
    for plan in env.plans(ident):
        inv = env.invoker(plan, env.s1)
        S.run_plan_deferred(plan, inv, env.s1, None, fill="zeros")  # ungated: S1, and the first-use allocations
        d = S.run_plan_deferred(plan, inv, env.s1, env.gate)         # gated: S1 and S2
        print("%-64s host %.3f ms, gate %.3f ms%s" % (plan.label, d.host_ms, env.gate.measured_ms,
                                                      " (may wait)" if S.may_wait(plan.label) else ""))
        ran += 1
    assert 1 <= ran <= 4


def _stream_prototypes(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return [m.group(1) for m in re.finditer(r"\b(amph_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, re.S)
            if "void* stream" in m.group(2)]


def test_both_tables_are_covered():
    """Every device entry of extent_cases.CALLS and every call of the batch
    headers that takes a stream is a case of test_call_follows_its_stream, and
    every pattern of the may-wait dict names plans that exist."""
    assert len(set(IDS)) == len(IDS)
    for c in X.CALLS:
        assert ("device" in c.modes) == (c.id in IDS), c.id
    batch = []
    for h in ("amphora_wire_batch.h", "amphora_upload_batch.h", "amphora_respond_batch.h"):
        batch += _stream_prototypes(h)
    assert sorted(batch) == sorted(name for name, _ in S.BATCH_CALLS) and len(batch) == 5
    names = {n for c in S.device_calls() for n in c.names}
    for n in _stream_prototypes("amphora.h"):  # every call of amphora.h that takes a stream to work on
        assert n in names or n == "amph_timing_event_record", n
    d = X.data(X.PIDS[0])
    waits = {c.id: [bool(S.may_wait(p.label)) for p in S.select(c, d)] for c in S.device_calls()}
    assert sorted(k for k, v in waits.items() if any(v)) == ["base64_decode", "mask_input_b64_more_secrets", "party_dev"]
    assert not all(waits["base64_decode"])  # without out_bytes the decode is held to S2
    labels = [p.label for c in S.device_calls() for p in S.select(c, d)]
    for pat in S.MAY_WAIT:
        assert any(re.search(pat, s) for s in labels), pat


# ---- chains with no host synchronisation ---------------------------------------------------
def _respond_then_verify(env):
    """Three parties' amph_odo_fields_b64_packed, then the client's
    amph_recombine_verify_b64_packed on their buffers and tables unchanged."""
    from tests import test_respond_batch as RB
    n = 3
    odos, y = RB.honest(n)
    o_fault, local, o_rej = 8, 200, 6  # a MAC fault in the 385-word object; party 0 rejects the 193-word one
    odos = FC.with_fault(odos, int(RB.WOFF[o_fault]) + local)
    toff, nchars = RB.slots(0)
    K, T, WOFF = RB.K, RB.T, RB.WOFF
    ins = [X.Arr("%s%d" % (X.FIELD[k], j), X.WORD, data=o[k]) for j, o in enumerate(odos) for k in range(5)]
    ins += [X.Arr("woff", X.OFFS, data=WOFF), X.Arr("toff", X.OFFS, data=toff),
            X.Arr("reject", X.VERDICT, data=np.array([17 if o == o_rej else X.NF for o in range(K)], np.int64))]
    outs = [X.Arr("t%s%d" % (X.FIELD[k], j), X.B64, n=nchars) for j in range(n) for k in range(5)]
    outs += [X.Arr("out", X.WORD, n=16 * T), X.Arr("ff", X.VERDICT, n=8 * K),
             X.Arr("bad", X.VERDICT, verdict=[0 if o == o_rej else -1 for o in range(K)])]

    def call(L, h, p, fl, s):
        for j in range(n):
            odo = env.A._lib._AmphOdo(*[p["%s%d" % (f, j)] for f in X.FIELD], 16 * T)
            ob = env.A._lib._AmphOdoB64Out(*[p["t%s%d" % (f, j)] for f in X.FIELD], nchars)
            st = L.amph_odo_fields_b64_packed(h, C.byref(odo), p["woff"], p["toff"], K, C.byref(ob),
                                              p["reject"] if j == 0 else None, fl, s)
            if st:
                return st
        arr = (env.A._lib._AmphOdoB64 * n)()
        for j in range(n):
            arr[j] = env.A._lib._AmphOdoB64(*[p["t%s%d" % (f, j)] for f in X.FIELD], nchars)
        return L.amph_recombine_verify_b64_packed(h, arr, n, p["woff"], p["toff"], K, p["out"], p["ff"], p["bad"],
                                                  fl, s)

    def check(whole):
        ff = np.frombuffer(whole["ff"], np.int64)
        for o in range(K):
            lo, hi = int(WOFF[o]), int(WOFF[o + 1])
            if o != o_rej:
                assert ff[o] == (local if o == o_fault else X.NF), ("first_fail", o, int(ff[o]))
            if o not in (o_rej, o_fault):
                assert whole["out"][16 * lo:16 * hi] == y[lo:hi].tobytes(), ("secrets", o)
            for j in range(n):  # the texts in between: Python's base64 of each object's words
                for k in range(5):
                    got = whole["t%s%d" % (X.FIELD[k], j)][int(toff[o]):int(toff[o]) + RB.nchars_of(hi - lo)]
                    if j == 0 and o == o_rej:
                        assert got[:4] == b"!!!!"
                    else:
                        assert got == base64.b64encode(odos[j][k][lo:hi].tobytes()), ("text", j, k, o)
    return X.Plan("chain odo_fields_b64_packed x%d -> recombine_verify_b64_packed" % n, ins, outs, call, check=check)


def _mask_then_convert(env):
    """The client's amph_mask_input_json_packed, then a party's
    amph_convert_share_json_packed reading out_text / out_text_offsets."""
    from tests import test_wire_batch as WB
    d, n, sizes = env.d, 3, S.BSIZES
    K, T = len(sizes), sum(sizes)
    woff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    o_fault, local = 3, 64
    od = d.odo_prefix(n, T, int(woff[o_fault]) + local)
    sec = d.secrets[:T]
    masked, _ = d.F.mask_input(sec, od)
    tup = np.ascontiguousarray(d.party(0)[1][:T])
    share = d.F.convert_share(np.ascontiguousarray(masked), tup, d.key, False)
    texts = [[[base64.b64encode(f[int(woff[o]):int(woff[o + 1])].tobytes()) for f in p_] for p_ in od]
             for o in range(K)]
    toff, nchars = WB.layout(sizes, "dense")
    bufs = WB.buffers(texts, sizes, toff, nchars)
    ooff, at = [], 0
    for o, W in enumerate(sizes):
        ooff.append(at)
        at += -(-(37 * W + 1 if W else 2) // 16) * 16 + 16 * (o % 3)
    cap = at
    ins = X.odo_arrs(bufs, X.B64) + [X.Arr("woff", X.OFFS, data=woff), X.Arr("toff", X.OFFS, data=toff),
                                     X.Arr("ooff", X.OFFS, data=np.array(ooff, np.uint64)),
                                     X.Arr("secrets", X.WORD, data=sec), X.Arr("tuples", X.WORD, data=tup)]
    verified = [o for o in range(K) if o != o_fault]
    outs = [X.Arr("text", X.WORD, n=cap), X.Arr("shares", X.WORD, n=32 * T),
            X.Arr("ff", X.VERDICT, verdict=[local if o == o_fault else -1 for o in range(K)]),
            X.Arr("bad", X.VERDICT, verdict=[-1] * K), X.Arr("cbad", X.VERDICT, n=8 * K)]
    key = FC.arr([d.key])[0].tobytes()

    def call(L, h, p, fl, s):
        st = L.amph_mask_input_json_packed(h, X.b64_struct(p, n, nchars), n, p["woff"], p["toff"], K, p["secrets"],
                                           p["text"], cap, p["ooff"], p["ff"], p["bad"], fl, s)
        return st or L.amph_convert_share_json_packed(h, p["text"], cap, p["woff"], p["ooff"], K, p["tuples"], key, 0,
                                                      p["shares"], p["cbad"], fl, s)

    def check(whole):
        cbad = np.frombuffer(whole["cbad"], np.int64)
        for o in verified:  # (the text of an object whose masks failed is not promised)
            lo, hi = int(woff[o]), int(woff[o + 1])
            assert cbad[o] == X.NF, ("bad_index", o, int(cbad[o]))
            assert whole["text"][ooff[o]:ooff[o] + (37 * (hi - lo) + 1 if hi > lo else 2)] == X.data_text(masked[lo:hi])
            assert whole["shares"][32 * lo:32 * hi] == share[lo:hi].tobytes(), ("share rows", o)
    return X.Plan("chain mask_input_json_packed -> convert_share_json_packed", ins, outs, call, check=check)


@pytest.mark.parametrize("chain", [_respond_then_verify, _mask_then_convert], ids=["respond-verify", "mask-convert"])
def test_chains_need_no_host_sync(env, chain):
    """Inputs deferred behind the gate, nothing synchronises between the calls
    of a chain, and the stream has not reached the first of them when the last
    has returned."""
    plan = chain(env)
    inv = env.invoker(plan, env.s1)
    S.run_plan_deferred(plan, inv, env.s1, None, fill="zeros")
    d = S.run_plan_deferred(plan, inv, env.s1, env.gate)
    assert d.reached is False
    print("%s: host %.3f ms" % (plan.label, d.host_ms))


# ---- execution order differs from enqueue order ----------------------------------------------
def run_inverted(env, plan_a, plan_b, ctx=None):
    """A enqueued first on s1 behind the gate, B second on s2 with no gate:
    B runs first.  Both satisfy S1; S2 is not asserted (growing a scratch may
    legitimately wait)."""
    a = S.Deferred(plan_a, env.s1, env.gate)
    b = S.Deferred(plan_b, env.s2, None)
    a.start()
    a.call(env.invoker(plan_a, env.s1, ctx))
    a.close()
    b.start()
    b.call(env.invoker(plan_b, env.s2, ctx))
    b.close()
    b.finish("second, no gate")
    a.finish("first, gated")
    return a, b


@pytest.mark.parametrize("ident", [c.id for c in S.device_calls()])
def test_execution_order_may_differ_from_enqueue_order(env, ident):
    call = next(c for c in S.device_calls() if c.id == ident)
    small, large = S.smallest_and_largest(call, env.d)
    run_inverted(env, small, large)


@pytest.mark.parametrize("first", ["encode", "decode"])
def test_exchange_scratch_grows_under_a_pending_call(env, first):
    """One fresh context: its exchange scratch is sized by call A, pending on
    s1 behind the gate, when call B on s2 needs a larger one."""
    enc = env.find("exchange_encode", "exchange_encode mixed npairs=1 align=3")
    dec = env.find("exchange_decode", "exchange_decode len=16385 align=1")
    enc_big = env.find("exchange_encode", "exchange_encode max npairs=1025 align=5")
    dec_small = env.find("exchange_decode", "exchange_decode len=15 align=9")
    ctx = env.context()
    if first == "encode":
        run_inverted(env, enc, dec, ctx)
    else:
        run_inverted(env, dec_small, enc_big, ctx)


def test_two_device_sessions_interleaved(env):
    """begin A, begin B, partner A, partner B, finish B, finish A on two
    streams of one context, A's stream gated."""
    L, d, n = env.L, env.d, 2
    plans = {W: env.find("party_dev", "party_dev n=%d W=%d" % (n, W)) for W in (1, 129)}
    a, b = S.Deferred(plans[1], env.s1, env.gate), S.Deferred(plans[129], env.s2, None)
    want = {}
    for W in (1, 129):
        (y, r, v, _, _), ow, ou = X._session_expect(d, n, W)
        want[W] = ([base64.b64encode(X.raw(x)) for x in (y, r, v, ow, ou)], d.pre_text(1, W))
    sess = {}
    try:
        def begin(x, W):
            p, ph = x.ptrs, C.c_void_p()
            st = L.amph_party_begin_dev(env.ctx._h, p["share"], 32, p["masks"], p["triples"], W, n, p["y"], p["r"],
                                        p["v"], C.c_void_p(x.stream.cuda_stream), C.byref(ph))
            assert st == X.OK, L.amph_last_error()
            sess[W] = ph

        def partner(x, W):
            st = L.amph_party_partner_dev(sess[W], 1, x.ptrs["text1"], len(want[W][1]), x.ptrs["bad1"],
                                          C.c_void_p(x.stream.cuda_stream))
            assert st == X.OK, L.amph_last_error()

        def finish(x, W):
            out = (C.c_void_p * 5)()
            st = L.amph_party_finish_b64_dev(sess[W], 1, out, C.c_void_p(x.stream.cuda_stream))
            assert st == X.OK, L.amph_last_error()
            return out
        a.start()
        b.start()
        begin(a, 1)
        begin(b, 129)
        partner(a, 1)
        partner(b, 129)
        fb = finish(b, 129)
        fa = finish(a, 1)
        a.status = b.status = X.OK
        reached = a.before.query()
        b.close()
        a.close()
        b.finish("session B, no gate")
        a.finish("session A, gated")
        assert not reached, "S2 (no wait): the six session calls returned after the gated stream had started"
        for W, out in ((129, fb), (1, fa)):
            for k in range(5):
                assert X._read_dev(out[k], len(want[W][0][k])) == want[W][0][k], ("session W=%d" % W, "field", k)
    finally:
        S.wait_event(_marker(env, env.s1), "session stream s1")
        S.wait_event(_marker(env, env.s2), "session stream s2")
        for ph in sess.values():
            L.amph_party_free(ph)


def _marker(env, stream):
    e = env.torch.cuda.Event()
    e.record(stream)
    return e


# ---- two threads, two streams, one context ---------------------------------------------------
ROTATION = [
    ("exchange_encode", "exchange_encode mixed npairs=257 align=5"),
    ("exchange_decode", "exchange_decode len=8193 align=1"),
    ("recombine_verify", "recombine_verify n=3 W=1025 fault=1024"),          # a lane call
    ("recombine_verify_b64", "recombine_verify_b64 n=3 W=193 fault=192"),    # a wire call
    ("recombine_verify_packed", "recombine_verify_packed n=3 T=1025 faults=(0, 1024)"),
    ("recombine_object", "recombine_object n=3 W=65"),                       # a ragged call
]


def test_two_threads_two_streams(env):
    """A stress, not a proof: two threads (ctypes releases the GIL during a
    call), each with its own side stream, run the gated S1 sequence 20 times
    over a fixed rotation of six calls on ONE context, the second thread three
    calls ahead of the first, and every result is checked."""
    plans = [env.find(i, label) for i, label in ROTATION]
    for p in plans:  # first-use allocations, once
        S.run_plan_deferred(p, env.invoker(p, env.s1), env.s1, None)
    errors = []

    def work(stream, shift):
        try:
            for i in range(20):
                p = plans[(i + shift) % len(plans)]
                S.run_plan_deferred(p, env.invoker(p, stream), stream, env.gate, no_wait=False)
        except BaseException as e:  # noqa: B902 -- reported by the test's thread
            errors.append((shift, e))
    t0 = time.monotonic()
    threads = [threading.Thread(target=work, args=(s, k)) for s, k in ((env.s1, 0), (env.s2, 3))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(4 * S.DEADLINE_S)
    assert not any(t.is_alive() for t in threads), "a thread did not finish"
    print("two threads: %.3f s" % (time.monotonic() - t0))
    if errors:
        raise errors[0][1]


# ---- captured in a graph and replayed ----------------------------------------------------------
W_GRAPH, N_GRAPH, FAULT_AT = 1025, 3, 64
CHAINS = ["mask_input", "recombine_verify", "recombine_verify_b64", "recombine_verify_packed"]


class Chain:
    """Three calls of one entry point on the same inputs into three outputs,
    as one linear chain on one stream; the inputs are rewritten in place."""

    def __init__(self, env, kind):
        torch = env.torch
        self.env, self.kind, self.offs = env, kind, X.packed_offsets(W_GRAPH)
        self.K = len(self.offs) - 1
        self.nv = self.K if kind.endswith("packed") else 1
        host = self.inputs(None)
        self.dev = {k: torch.zeros(len(v), dtype=torch.uint8, device="cuda") for k, v in host.items()}
        self.pin = {k: torch.empty(len(v), dtype=torch.uint8).pin_memory() for k, v in host.items()}
        self.out = [torch.zeros(16 * W_GRAPH, dtype=torch.uint8, device="cuda") for _ in range(3)]
        self.ff = torch.zeros(self.nv, dtype=torch.int64, device="cuda")
        self.bad = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.back = [torch.empty(16 * W_GRAPH, dtype=torch.uint8).pin_memory() for _ in range(3)]
        self.vback = torch.empty(self.nv + 1, dtype=torch.int64).pin_memory()

    def od(self, fault):
        return self.env.d.odo_prefix(N_GRAPH, W_GRAPH, fault)

    def inputs(self, fault):
        od = self.od(fault)
        if self.kind == "recombine_verify_b64":
            od = X.texts_of(od)
        host = {"%s%d" % (X.FIELD[k], j): X.raw(o[k]) for j, o in enumerate(od) for k in range(5)}
        host["secrets"] = X.raw(self.env.d.secrets[:W_GRAPH])
        host["offsets"] = X.raw(np.array(self.offs, np.uint64))
        return host

    def expected(self, fault):
        d, od = self.env.d, self.od(fault)
        y, ff = d.F.recombine_verify(od)
        assert ff == (-1 if fault is None else fault)
        out = X.raw(y)
        if self.kind == "mask_input":  # the masked words of a call that verified
            out = X.raw(d.F.mask_input(d.secrets[:W_GRAPH], od)[0]) if fault is None else None
        if self.kind.endswith("packed"):
            verdicts = []
            for o in range(self.K):
                lo, hi = self.offs[o], self.offs[o + 1]
                verdicts.append(-1 if hi == lo else d.F.recombine_verify([tuple(f[lo:hi] for f in p_) for p_ in od])[1])
        else:
            verdicts = [ff]
        return out, [X.NF if v < 0 else v for v in verdicts]

    def issue(self, stream):
        L, h, s = self.env.L, self.env.ctx._h, C.c_void_p(stream.cuda_stream)
        p = {k: t.data_ptr() for k, t in self.dev.items()}
        ff, bad = self.ff.data_ptr(), self.bad.data_ptr()
        nchars = 4 * ((16 * W_GRAPH + 2) // 3)
        for k in range(3):
            out = self.out[k].data_ptr()
            if self.kind == "mask_input":
                st = L.amph_mask_input(h, X.odo_struct(p, N_GRAPH, 16 * W_GRAPH), N_GRAPH, p["secrets"], W_GRAPH, out,
                                       X.i64(ff), X.F_DEVICE | F_ACCUMULATE, s)
            elif self.kind == "recombine_verify":
                st = L.amph_recombine_verify(h, X.odo_struct(p, N_GRAPH, 16 * W_GRAPH), N_GRAPH, out, X.i64(ff),
                                             X.F_DEVICE | F_ACCUMULATE, s)
            elif self.kind == "recombine_verify_b64":
                st = L.amph_recombine_verify_b64(h, X.b64_struct(p, N_GRAPH, nchars), N_GRAPH, W_GRAPH, out,
                                                 X.i64(ff), X.i64(bad), X.F_DEVICE, s)
            else:
                st = L.amph_recombine_verify_packed(h, X.odo_struct(p, N_GRAPH, 16 * W_GRAPH), N_GRAPH, p["offsets"],
                                                    self.K, out, ff, X.F_DEVICE, s)
            assert st == X.OK, (self.kind, k, st, L.amph_last_error())

    def rewrite(self, fault):
        """On the current stream: the inputs in place, the verdict words reset,
        the outputs cleared."""
        for k, v in self.inputs(fault).items():
            self.pin[k].copy_(self.env.torch.frombuffer(bytearray(v), dtype=self.env.torch.uint8))
            self.dev[k].copy_(self.pin[k], non_blocking=True)
        self.ff.fill_(X.NF)
        self.bad.fill_(X.NF)
        for o in self.out:
            o.zero_()

    def read(self):
        """On the current stream -> an event behind the copies back."""
        for k in range(3):
            self.back[k].copy_(self.out[k], non_blocking=True)
        self.vback[:self.nv].copy_(self.ff, non_blocking=True)
        self.vback[self.nv:].copy_(self.bad, non_blocking=True)
        e = self.env.torch.cuda.Event()
        e.record()
        return e

    def check(self, fault, tag):
        out, verdicts = self.expected(fault)
        got = [int(v) for v in self.vback.numpy()]
        assert got[:self.nv] == verdicts and got[self.nv] == X.NF, (self.kind, tag, "verdicts", got, verdicts)
        for k in range(3):
            if out is not None:
                assert self.back[k].numpy().tobytes() == out, (self.kind, tag, "output of call", k)


@pytest.mark.parametrize("kind", CHAINS)
def test_captured_steps_replay(env, kind):
    """Three device-mode calls captured as one linear chain on one stream and
    replayed twice on inputs rewritten in place: honest, then a MAC fault at
    word 64.  The verdict words are reset on the same stream outside the
    graph; outputs and verdicts equal the oracle's both times."""
    torch = env.torch
    c, s = Chain(env, kind), env.s1
    with torch.cuda.stream(s):  # uncaptured first: first-use allocations, and the chain itself
        c.rewrite(FAULT_AT)
        c.issue(s)
        done = c.read()
    S.wait_event(done, kind)
    c.check(FAULT_AT, "uncaptured")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        c.issue(s)
    for fault in (None, FAULT_AT):
        with torch.cuda.stream(s):
            c.rewrite(fault)
            g.replay()
            done = c.read()
        S.wait_event(done, kind)
        c.check(fault, "replay, fault=%s" % fault)
