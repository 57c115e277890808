"""The stream contract and the buffer extents of the device-mode party batch
session (amph_parties_*_dev, include/amphora_party_batch.h), through the
harnesses of tests/stream_cases.py and tests/extent_cases.py with plans
defined here.

One plan: party 0 of three over objects of 1, 0, 64, 65 and 130 words runs
begin, both partners and finish_b64 on the caller's stream and copies its K
texts and its 5 K field texts (device to device, on the same stream) into
arrays of the arena.  The partners' text buffers carry Jackson's texts of the
oracle's diffs at the session's offsets, and FactorPair fragments and bare
colons in every gap and slot rest.

  S1 (order)    everything the calls enqueued ran behind the input copy and
                before the output copy: the image copied back holds the
                oracle's y / r / v, texts, verdicts and fields.
  S2 (no wait)  begin, partner, partner and finish together returned before
                the stream had passed the gate.  amph_parties_free is the one
                waiting call: the sessions are freed after the plan is done.
  extents       guard bands around every caller array (and the hostile gaps
                inside the text buffers) are unchanged, the inputs are
                unchanged, and no output depends on the bytes around the inputs
                (extent_cases.run_plan's P1-P4, zeros and hostile surrounds).
"""
import ctypes as C

import numpy as np
import pytest

from tests import extent_cases as X
from tests import stream_cases as S

pytestmark = pytest.mark.gpu

COUNTS = [1, 0, 64, 65, 130]
N = 3
_FRAG = b',{"a":1,"b":2}:'


class Env:
    def __init__(self):
        import torch
        import amphora_amd as A
        from oracle import amphora_oracle as O
        from oracle import coracle
        from tests.test_party_batch import Case
        self.torch, self.A, self.L = torch, A, A._lib.lib
        self.ctx = A.Context(O.TEST_PRIME, O.TEST_R, O.TEST_RINV)
        self.case = Case(coracle.test_field(threads=8), N, COUNTS)
        self.gate = S.Gate()
        self.stream = torch.cuda.Stream()
        self.live = []  # sessions, freed after their plan is done (the free waits)

    def free(self):
        for ph in self.live:
            self.L.amph_parties_free(ph)
        self.live = []


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.free()


def build_plan(env):
    A, c = env.A, env.case
    K, T = len(COUNTS), c.T
    toff = np.concatenate([[0], np.cumsum([A._lib.exchange_slot_chars(2 * w) for w in COUNTS])]).astype(np.uint64)
    foff = np.concatenate([[0], np.cumsum([A._lib.wire_slot_chars(w) for w in COUNTS])]).astype(np.uint64)
    text_bytes, field_chars = int(toff[-1]), int(foff[-1])
    own, want_fields = c.texts(0), c.fields(0)
    ins = [X.Arr("share", X.WORD, data=X.raw(c.shares[0])), X.Arr("masks", X.WORD, data=X.raw(c.masks[0])),
           X.Arr("triples", X.WORD, data=X.raw(c.triples[0]))]
    for k in (1, 2):
        texts = c.texts(k)
        buf = np.frombuffer((_FRAG * (text_bytes // len(_FRAG) + 1))[:text_bytes], np.uint8).copy()
        for o, t in enumerate(texts):  # hostile fragments stay in every gap and slot rest
            buf[int(toff[o]):int(toff[o]) + len(t)] = np.frombuffer(t, np.uint8)
        ins.append(X.Arr("texts%d" % k, X.XCHG, data=buf.tobytes(), offset=0))
        ins.append(X.Arr("lens%d" % k, X.OFFS, data=np.array([len(t) for t in texts], np.uint64).tobytes()))
    outs = [X.Arr(nm, X.WORD, n=16 * T, expect=X.raw(c.pre[0][i])) for i, nm in enumerate("yrv")]
    outs += [X.Arr("bad%d" % k, X.VERDICT, verdict=[-1] * K) for k in (1, 2)]
    outs += [X.Arr("text", X.XCHG, n=text_bytes, offset=0)]
    outs += [X.Arr("f%d" % k, X.B64, n=field_chars) for k in range(5)]
    wo = c.woff.copy()

    def call(L, h, p, fl, s):
        ph = C.c_void_p()
        st = L.amph_parties_begin_dev(h, p["share"], 32, p["masks"], p["triples"], wo.ctypes.data, K, N, p["y"],
                                      p["r"], p["v"], s, C.byref(ph))
        if st:
            return st
        env.live.append(ph)
        for k in (1, 2):
            st = L.amph_parties_partner_dev(ph, k, p["texts%d" % k], p["lens%d" % k], p["bad%d" % k], s)
            if st:
                return st
        out = (C.c_void_p * 5)()
        st = L.amph_parties_finish_b64_dev(ph, 1, out, s)
        if st:
            return st
        tp, op, lp = C.c_void_p(), C.c_void_p(), C.c_void_p()
        st = L.amph_parties_text_dev(ph, C.byref(tp), C.byref(op), C.byref(lp))
        if st:
            return st
        # device-to-device copies on the current (the plan's) stream: they only enqueue.  Text by text: what
        # lies between the texts in the session's buffers is never written, so it is not the call's output
        view = A._lib._dev_view
        dst = [view(p["text"], text_bytes, "|u1", 0)] + [view(p["f%d" % k], field_chars, "|u1", 0) for k in range(5)]
        src = [view(tp.value, text_bytes, "|u1", 0)] + [view(out[k], field_chars, "|u1", 0) for k in range(5)]
        for o in range(K):
            a, n = int(toff[o]), len(own[o])
            dst[0][a:a + n].copy_(src[0][a:a + n], non_blocking=True)
            a, n = int(foff[o]), len(want_fields[o][0])
            for k in range(5):
                if n:
                    dst[1 + k][a:a + n].copy_(src[1 + k][a:a + n], non_blocking=True)
        return X.OK

    def check(whole):
        for o in range(K):
            a = int(toff[o])
            assert whole["text"][a:a + len(own[o])] == own[o], "object %d's own text" % o
            for k in range(5):
                a = int(foff[o])
                assert whole["f%d" % k][a:a + len(want_fields[o][k])] == want_fields[o][k], (o, k)
    return X.Plan("parties_dev n=%d K=%d T=%d" % (N, K, T), ins, outs, call, check=check)


def invoker(env, plan, stream_handle):
    def invoke(ins, outs):
        p = {k: g.ptr for k, g in list(ins.items()) + list(outs.items())}
        return plan.call(env.L, env.ctx._h, p, X.F_DEVICE, stream_handle)
    return invoke


def test_the_dev_calls_follow_their_stream_and_do_not_wait(env):
    plan = build_plan(env)
    inv = invoker(env, plan, C.c_void_p(env.stream.cuda_stream))
    S.run_plan_deferred(plan, inv, env.stream, None, fill="zeros")  # ungated: S1, and the first-use allocations
    env.free()  # (the buffers go to the pool: the gated run allocates nothing)
    d = S.run_plan_deferred(plan, inv, env.stream, env.gate, no_wait=True)  # gated: S1 and S2
    assert d.reached is False
    print("%s: host %.3f ms, gate %.3f ms" % (plan.label, d.host_ms, env.gate.measured_ms))
    env.free()


def test_nothing_outside_the_callers_arrays_is_written_and_inputs_are_unchanged(env):
    plan = build_plan(env)
    torch = env.torch
    with torch.cuda.stream(env.stream):
        inv = invoker(env, plan, C.c_void_p(env.stream.cuda_stream))
        got = X.run_plan(plan, True, inv, sync=env.stream.synchronize)
    assert set(got) >= {"y", "r", "v", "bad1", "bad2", "text"}
    env.free()
