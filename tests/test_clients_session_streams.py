"""The stream contract and the buffer extents of the device-mode client
session for K secrets (amph_clients_*_dev, include/amphora_client_batch.h),
through the harnesses of tests/stream_cases.py and tests/extent_cases.py with
plans defined here.

A plan: three parties' slotted field buffers (the gaps between the texts hold
'!') of the objects [0, 1, 192, 0, 193, 2] or of one object go into a session
in the order 2, 0, 1 on the caller's stream, then one of the three finish
calls; every object is a slice of the C oracle's rows (extent_cases.Data), so
the references are slices of the oracle's results.

  S1 (order)    everything the calls enqueued ran behind the input copy and
                before the output copy: the image copied back holds the
                oracle's secrets / masked words / records / framed texts and
                the K verdict words of every party call and of the finish.
  S2 (no wait)  begin, the three party calls and the finish together returned
                before the stream had passed the gate.  amph_clients_free is
                the one waiting call: sessions are freed after the plan is done.
  extents       guard bands around every caller array are unchanged, the
                inputs are unchanged, and no output depends on the bytes around
                the inputs (extent_cases.run_plan's P1-P4).
"""
import base64
import ctypes as C

import numpy as np
import pytest

from tests import extent_cases as X
from tests import stream_cases as S

pytestmark = pytest.mark.gpu

TABLES = {"six": [0, 1, 192, 0, 193, 2], "one": [193]}
N = 3
ORDER = (2, 0, 1)
FINISHES = ("verify", "mask", "mask_json")


def chars(W):
    return 4 * ((16 * W + 2) // 3)


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
            self.L.amph_clients_free(h)
        self.live = []


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.free()


def build_plan(env, table, finish, fault=None):
    d = env.d
    sizes = TABLES[table]
    K, T = len(sizes), sum(sizes)
    woff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    foff = np.concatenate([[0], np.cumsum([(chars(W) + 15) & ~15 for W in sizes])]).astype(np.int64)
    ulen = [37 * W + 1 if W else 2 for W in sizes]
    uoff = np.concatenate([[0], np.cumsum([(u + 15) & ~15 for u in ulen])]).astype(np.int64)
    od = d.odo_prefix(N, T, fault)  # fault: a global word; its object reports it with its own index
    y, _ = d.F.recombine_verify(od)
    sec = d.secrets[:T]
    m, _ = d.F.mask_input(sec, od)
    ffs = [-1] * K
    if fault is not None:
        o = max(o for o in range(K) if woff[o] <= fault)
        ffs[o] = int(fault - woff[o])
    nchars = int(foff[-1])
    ins = []
    for j in range(N):
        for k in range(5):
            buf = np.full(nchars, ord("!"), np.uint8)  # never read outside the texts
            for o, W in enumerate(sizes):
                a = int(woff[o])
                t = np.frombuffer(base64.b64encode(X.raw(od[j][k][a:a + W])), np.uint8)
                buf[foff[o]:foff[o] + t.size] = t
            ins.append(X.Arr("%s%d" % (X.FIELD[k], j), X.B64, data=buf))
    outs = [X.Arr("bad%d" % j, X.VERDICT, verdict=[-1] * K) for j in range(N)]
    outs += [X.Arr("ff", X.VERDICT, verdict=ffs), X.Arr("bad", X.VERDICT, verdict=[-1] * K)]
    check = None
    if finish == "verify":
        # (the failing object's secrets are unspecified only in that they fail the MAC: K_RV writes them)
        outs.append(X.Arr("out", X.WORD, n=16 * T, expect=X.raw(y)))
    else:
        ins.append(X.Arr("secrets", X.WORD, data=sec))
        if finish == "mask":
            outs.append(X.Arr("o16", X.WORD, n=16 * T, expect=X.raw(m)))
            outs.append(X.Arr("o24", X.REC24, n=24 * T, offset=X.OFFSET[X.WORD],
                              expect=b"".join(base64.b64encode(X.raw(w)) for w in m)))
        else:
            outs.append(X.Arr("text", X.JSONTXT, n=int(uoff[-1]), offset=X.OFFSET[X.B64]))

            def check(whole):
                for o, W in enumerate(sizes):
                    a = int(woff[o])
                    got = whole["text"][uoff[o]:uoff[o] + ulen[o]]
                    assert got == X.data_text(m[a:a + W]), "object %d's framed text" % o

    def call(L, h, p, fl, s):
        ch = C.c_void_p()
        st = L.amph_clients_begin_dev(h, woff.ctypes.data, K, N, s, C.byref(ch))
        if st:
            return st
        env.live.append(ch)
        for j in ORDER:
            one = X.b64_struct({"%s0" % f: p["%s%d" % (f, j)] for f in X.FIELD}, 1, nchars)
            st = L.amph_clients_party_dev(ch, j, one, p["bad%d" % j], s)
            if st:
                return st
        if finish == "verify":
            return L.amph_clients_finish_verify_dev(ch, p["out"], p["ff"], p["bad"], s)
        if finish == "mask":
            return L.amph_clients_finish_mask_dev(ch, p["secrets"], p["o16"], p["o24"], p["ff"], p["bad"], s)
        return L.amph_clients_finish_mask_json_dev(ch, p["secrets"], p["text"], int(uoff[-1]), p["ff"], p["bad"], s)

    return X.Plan("clients_dev %s n=%d %s fault=%s" % (finish, N, table, fault), ins, outs, call, check=check)


def invoker(env, plan, stream_handle):
    def invoke(ins, outs):
        p = {k: g.ptr for k, g in list(ins.items()) + list(outs.items())}
        return plan.call(env.L, env.ctx._h, p, X.F_DEVICE, stream_handle)
    return invoke


@pytest.mark.parametrize("finish", FINISHES)
@pytest.mark.parametrize("table", list(TABLES))
def test_the_dev_calls_follow_their_stream_and_do_not_wait(env, table, finish):
    plan = build_plan(env, table, finish)
    inv = invoker(env, plan, C.c_void_p(env.stream.cuda_stream))
    S.run_plan_deferred(plan, inv, env.stream, None, fill="zeros")  # ungated: S1, and the first-use allocations
    env.free()  # (the buffer goes to the pool: the gated run allocates nothing but the session's pinned table)
    d = S.run_plan_deferred(plan, inv, env.stream, env.gate, no_wait=True)  # gated: S1 and S2
    assert d.reached is False
    print("%s: host %.3f ms, gate %.3f ms" % (plan.label, d.host_ms, env.gate.measured_ms))
    env.free()


@pytest.mark.parametrize("finish", FINISHES)
@pytest.mark.parametrize("table", list(TABLES))
def test_nothing_outside_the_callers_arrays_is_written_and_inputs_are_unchanged(env, table, finish):
    torch = env.torch
    T = sum(TABLES[table])
    for fault in (None, T - 1):
        plan = build_plan(env, table, finish, fault)
        with torch.cuda.stream(env.stream):
            inv = invoker(env, plan, C.c_void_p(env.stream.cuda_stream))
            got = X.run_plan(plan, True, inv, sync=env.stream.synchronize)
        assert set(got) >= {"ff", "bad", "bad0", "bad1", "bad2"}
        env.free()
