"""The stream contract and the buffer extents of the device-mode client
session (amph_client_*_dev, include/amphora_client_session.h), through the
harnesses of tests/stream_cases.py and tests/extent_cases.py with plans
defined here.

A plan: three parties' base64 texts of 1, 64 or 193 words go into a session
in the order 2, 0, 1 on the caller's stream, then one of the three finish
calls; references are the C oracle's (extent_cases.Data).

  S1 (order)    everything the calls enqueued ran behind the input copy and
                before the output copy: the image copied back holds the
                oracle's secrets / masked words / records / framed text and
                the verdict words of every party call and of the finish.
  S2 (no wait)  begin, the three party calls and the finish together returned
                before the stream had passed the gate.  amph_client_free is
                the one waiting call: sessions are freed after the plan is done.
  extents       guard bands around every caller array are unchanged, the
                inputs are unchanged, and no output depends on the bytes around
                the inputs (extent_cases.run_plan's P1-P4).
"""
import base64
import ctypes as C

import pytest

from tests import extent_cases as X
from tests import stream_cases as S

pytestmark = pytest.mark.gpu

COUNTS = [1, 64, 193]
N = 3
ORDER = (2, 0, 1)
FINISHES = ("verify", "mask", "mask_json")


class Env:
    def __init__(self):
        import torch
        import amphora_amd as A
        self.torch, self.A, self.L = torch, A, A._lib.lib
        self.d = X.data(X.PIDS[0])
        self.ctx = A.Context(self.d.pr.p, self.d.pr.r, self.d.pr.rinv)
        self.gate = S.Gate()
        self.stream = torch.cuda.Stream()
        self.live = []  # sessions, freed after their plan is done (the free waits)

    def free(self):
        for h in self.live:
            self.L.amph_client_free(h)
        self.live = []


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.free()


def build_plan(env, W, finish, fault=None):
    d = env.d
    od = d.odo_prefix(N, W, fault)
    tx = X.texts_of(od)
    nchars = tx[0][0].size
    y, ff = d.F.recombine_verify(od)
    sec = d.secrets[:W]
    ins = X.odo_arrs(tx, X.B64)
    outs = [X.Arr("bad%d" % j, X.VERDICT, verdict=-1) for j in range(N)]
    outs += [X.Arr("ff", X.VERDICT, verdict=ff), X.Arr("bad", X.VERDICT, verdict=-1)]
    if finish == "verify":
        outs.append(X.Arr("out", X.WORD, n=16 * W, expect=X.raw(y)))
    else:
        ins.append(X.Arr("secrets", X.WORD, data=sec))
        m, _ = d.F.mask_input(sec, od)
        if finish == "mask":
            outs.append(X.Arr("o16", X.WORD, n=16 * W, expect=X.raw(m) if fault is None else None))
            outs.append(X.Arr("o24", X.REC24, n=24 * W, offset=X.OFFSET[X.WORD],
                              expect=b"".join(base64.b64encode(X.raw(w)) for w in m) if fault is None else None))
        else:
            text = X.data_text(m)
            outs.append(X.Arr("text", X.JSONTXT, n=len(text), offset=X.OFFSET[X.B64],
                              expect=text if fault is None else None))

    def call(L, h, p, fl, s):
        ch = C.c_void_p()
        st = L.amph_client_begin_dev(h, W, N, s, C.byref(ch))
        if st:
            return st
        env.live.append(ch)
        for j in ORDER:
            one = X.b64_struct({"%s0" % f: p["%s%d" % (f, j)] for f in X.FIELD}, 1, nchars)
            st = L.amph_client_party_dev(ch, j, one, X.i64(p["bad%d" % j]), s)
            if st:
                return st
        if finish == "verify":
            return L.amph_client_finish_verify_dev(ch, p["out"], X.i64(p["ff"]), X.i64(p["bad"]), s)
        if finish == "mask":
            return L.amph_client_finish_mask_dev(ch, p["secrets"], W, p["o16"], p["o24"], X.i64(p["ff"]),
                                                 X.i64(p["bad"]), s)
        return L.amph_client_finish_mask_json_dev(ch, p["secrets"], W, p["text"], 37 * W + 1, X.i64(p["ff"]),
                                                  X.i64(p["bad"]), s)

    return X.Plan("client_dev %s n=%d W=%d fault=%s" % (finish, N, W, fault), ins, outs, call)


def invoker(env, plan, stream_handle):
    def invoke(ins, outs):
        p = {k: g.ptr for k, g in list(ins.items()) + list(outs.items())}
        return plan.call(env.L, env.ctx._h, p, X.F_DEVICE, stream_handle)
    return invoke


@pytest.mark.parametrize("finish", FINISHES)
@pytest.mark.parametrize("W", COUNTS)
def test_the_dev_calls_follow_their_stream_and_do_not_wait(env, W, finish):
    plan = build_plan(env, W, finish)
    inv = invoker(env, plan, C.c_void_p(env.stream.cuda_stream))
    S.run_plan_deferred(plan, inv, env.stream, None, fill="zeros")  # ungated: S1, and the first-use allocations
    env.free()  # (the buffer goes to the pool: the gated run allocates nothing)
    d = S.run_plan_deferred(plan, inv, env.stream, env.gate, no_wait=True)  # gated: S1 and S2
    assert d.reached is False
    print("%s: host %.3f ms, gate %.3f ms" % (plan.label, d.host_ms, env.gate.measured_ms))
    env.free()


@pytest.mark.parametrize("finish", FINISHES)
@pytest.mark.parametrize("W", COUNTS)
def test_nothing_outside_the_callers_arrays_is_written_and_inputs_are_unchanged(env, W, finish):
    torch = env.torch
    for fault in (None, W - 1):
        plan = build_plan(env, W, finish, fault)
        with torch.cuda.stream(env.stream):
            inv = invoker(env, plan, C.c_void_p(env.stream.cuda_stream))
            got = X.run_plan(plan, True, inv, sync=env.stream.synchronize)
        assert set(got) >= {"ff", "bad", "bad0", "bad1", "bad2"}
        env.free()
