"""The stream contract of the device-mode calls (include/amphora.h "Memory"
and "Streams", the three batch headers' AMPH_F_DEVICE paragraphs): a call with
AMPH_F_DEVICE only enqueues work on the caller's stream and returns.

run_plan_deferred() runs one device-mode plan of tests/extent_cases.py (or of
BATCH_CALLS below) so that luck cannot order it:

  * the device arena holds ZEROS when the call is made -- "not there yet": all
    zero words, offset tables and texts give a wrong answer and no address
    outside the arena;
  * on a side stream (never the default one) a time-based gate runs first
    (torch.cuda._sleep, calibrated once per module by Gate), then the copy of
    the real image from page-locked memory, an event `before`, the call, the
    copy of the arena back to page-locked memory and an event `done`;
  * the host polls `done` against DEADLINE_S -- no wait here is unbounded.

Two properties:

  S1 (order)    P1-P3 of extent_cases hold on the image copied back: every
                launch, memset and copy of the call ran on the stream behind
                the input copy and before the output copy, or on a stream
                correctly chained to it.
  S2 (no wait)  `before` had not been reached when the call returned: the call
                cannot have waited for its stream or for the device.  Asserted
                on a plan's second run (an ungated first run takes the
                first-use allocations), and not for the plans of MAY_WAIT.

The gate is time-based because one the host releases would deadlock against
the library's legitimate hipEventSynchronize (the exchange scratch's growth).
Its length is no pass threshold: too short a gate fails S2, it never passes
it.  Target GATE_MS = 10 ms (23.76 M cycles measured 9.91 ms on the MI355X).
The host-side enqueue time it has to exceed, measured there on the library as
it was before these tests: 0.005-0.037 ms for a single call, at most 0.054 ms
for a selected plan (recombine_object with 5 ragged parties: two launches and
a stream-ordered allocation) and 0.056 ms for a chain of four calls --
ENQUEUE_MS = 0.06 ms.  Ten times that is 0.6 ms; the 10 ms target leaves a
further factor of 16 for a slower host.

References come from the plans (the C oracle, Python ints, base64, json),
never from another call into the library.  Importable without a GPU; the
tables are built on first use.
"""
from __future__ import annotations

import re
import time

import numpy as np

from tests import extent_cases as X

GATE_MS = 10.0        # target gate
GATE_CAP_MS = 50.0
ENQUEUE_MS = 0.06     # the slowest selected plan's host-side enqueue time (measured, module docstring)
DEADLINE_S = 10.0     # every wait for the GPU in these tests

# Plans that synchronise by contract: label pattern -> the header lines that say so.
# S1 applies to them, S2 does not.  At most 4 entries.
MAY_WAIT = {
    r"^base64_decode .* out_bytes=True$":
        "amphora.h:421-424 (with out_bytes non-null the call reads the last 2 chars back: a stream synchronisation)",
    r"^mask_input_b64 S>W ":
        "amphora.h:472-478 (n_secrets > words: device mode waits for the verdicts on that path)",
    r"^party_dev ":
        "amphora.h:610-611 (amph_party_free waits for the session's stream; the table entry frees its session)",
}
assert len(MAY_WAIT) <= 4


def may_wait(label: str):
    for pat, why in MAY_WAIT.items():
        if re.search(pat, label):
            return why
    return None


def wait_event(ev, what: str, deadline_s: float = DEADLINE_S):
    """Poll an event against a deadline: a step that never ends fails the test."""
    end = time.monotonic() + deadline_s
    while not ev.query():
        if time.monotonic() > end:
            raise AssertionError("%s: the GPU did not get there within %.0f s" % (what, deadline_s))
        time.sleep(0)


class Gate:
    """cycles of torch.cuda._sleep for about target_ms, measured with two
    events on a side stream; fails loudly outside [0.5, 5] x target."""

    PROBE = 1_000_000

    def __init__(self, target_ms: float = GATE_MS):
        import torch
        self.target_ms = target_ms
        self._s = torch.cuda.Stream()
        self.time(self.PROBE)  # the first launch pays for loading the kernel
        probe_ms = self.time(self.PROBE)
        assert probe_ms > 0, "the gate's probe took no time"
        self.cycles = max(1, int(self.PROBE * target_ms / probe_ms))
        self.measured_ms = self.time(self.cycles)
        lo, hi = 0.5 * target_ms, min(5 * target_ms, GATE_CAP_MS)
        assert lo <= self.measured_ms <= hi, "gate calibration: %d cycles took %.3f ms, outside [%.1f, %.1f] ms" % (
            self.cycles, self.measured_ms, lo, hi)

    def time(self, cycles: int) -> float:
        import torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self._s):
            e0.record()
            torch.cuda._sleep(cycles)
            e1.record()
        wait_event(e1, "gate calibration")
        return e0.elapsed_time(e1)

    def enqueue(self):
        """On the current stream."""
        import torch
        torch.cuda._sleep(self.cycles)


class DeferredArena(X.Arena):
    """A device Arena whose bytes are not there yet: commit() leaves zeros on
    the device and the image in page-locked memory; upload() / download()
    enqueue the copies on the current stream."""

    def __init__(self):
        super().__init__(True)
        self.image = self.back = None

    def commit(self):
        import torch
        img = np.zeros(max(self.size, 256), np.uint8)
        for g in self.items:
            img[g.start:g.start + g.size] = g.before
        self.image = torch.from_numpy(img).pin_memory()
        self.back = torch.empty_like(self.image).pin_memory()
        self.t = torch.zeros(img.size, dtype=torch.uint8, device="cuda")
        zeroed = torch.cuda.Event()
        zeroed.record()
        wait_event(zeroed, "zero fill of the arena")
        self.base = self.t.data_ptr()
        assert self.base % 256 == 0
        return self

    def upload(self):
        self.t.copy_(self.image, non_blocking=True)

    def download(self):
        self.back.copy_(self.t, non_blocking=True)

    def fetch(self):
        img = self.back.numpy()
        for g in self.items:
            g.after = img[g.start:g.start + g.size]


class Deferred:
    """One plan on `stream`: the constructor builds the arenas (zeros on the
    device, nothing enqueued); start() enqueues the gate (None: no gate), the
    input copy and `before`; call() makes the call and reads before.query();
    close() enqueues the copy back and `done`; finish() waits for `done` and
    asserts S1."""

    def __init__(self, plan, stream, gate, fill="hostile"):
        import torch
        self.plan, self.stream, self.gate = plan, stream, gate
        self.main, self.aux = DeferredArena(), X.Arena(False)
        self.ins = {a.name: (self.aux if a.host else self.main).add(a.name, a.kind, data=a.data, offset=a.offset,
                                                                     fill=fill) for a in plan.ins}
        self.outs = {a.name: (self.aux if a.host else self.main).add(a.name, a.kind, n=a.n, offset=a.offset)
                     for a in plan.outs}
        self.main.commit()
        self.aux.commit()
        prepare = getattr(plan, "prepare", None)
        if prepare:
            prepare(self.ins, self.outs)
        self.ptrs = {k: g.ptr for k, g in list(self.ins.items()) + list(self.outs.items())}
        self.before, self.done = torch.cuda.Event(), torch.cuda.Event()
        self.status = self.reached = self.host_ms = None

    def start(self):
        import torch
        with torch.cuda.stream(self.stream):
            if self.gate is not None:
                self.gate.enqueue()
            self.main.upload()
            self.before.record()
        return self

    def call(self, invoke):
        """invoke(ins, outs) -> status, as run_plan's."""
        import torch
        with torch.cuda.stream(self.stream):
            t0 = time.perf_counter()
            self.status = invoke(self.ins, self.outs)
            self.host_ms = 1e3 * (time.perf_counter() - t0)
        self.reached = self.before.query()
        return self.status

    def close(self):
        import torch
        with torch.cuda.stream(self.stream):
            self.main.download()
            self.done.record()

    def finish(self, tag="gated"):
        wait_event(self.done, self.plan.label)
        self.main.fetch()
        self.aux.fetch()
        try:
            return X.check_plan(self.plan, True, self.status, self.ins, self.outs, "%s [%s]" % (self.plan.label, tag))
        except AssertionError as e:
            raise AssertionError("S1 (order): %s" % e) from None

    def check_no_wait(self):
        assert self.gate is not None
        assert not self.reached, (
            "S2 (no wait): %s: the stream had passed the gate when the call returned -- the call took %.3f ms on the "
            "host, the gate is %.3f ms" % (self.plan.label, self.host_ms, self.gate.measured_ms))


def run_plan_deferred(plan, invoke, stream, gate, fill="hostile", no_wait=None):
    """S1, and S2 when `gate` is given and the plan is not in MAY_WAIT
    (no_wait overrides).  Returns the Deferred (host_ms, reached)."""
    d = Deferred(plan, stream, gate, fill).start()
    d.call(invoke)
    d.close()
    d.finish("gated" if gate is not None else "ungated")
    if no_wait is None:
        no_wait = gate is not None and may_wait(plan.label) is None
    if no_wait:
        d.check_no_wait()
    return d


# ---- selection from extent_cases.CALLS ---------------------------------------------------
_SIZE = re.compile(r"\b(W|T|npairs|nbytes|len|count)=(\d+)")
_PARTIES = re.compile(r"\bn=(\d+)")


def _key(label):
    n, m = _PARTIES.search(label), _SIZE.search(label)
    return (int(n.group(1)) if n else None, int(m.group(2)) if m else None)


def select(call, d):
    """At most four plans of one table entry: the smallest and the largest
    size, at the first and the last party count where the entry has one.  An
    entry yields several variants per (parties, size) -- faults, alignments,
    output choices; with c such corners 4 // c of them are taken from each,
    spread evenly from the last one backwards, so that the honest and the
    faulted, the waiting and the non-waiting variants all occur."""
    groups = {}
    for plan in call.gen(d):
        groups.setdefault(_key(plan.label), []).append(plan)
    ns = sorted({k[0] for k in groups if k[0] is not None}) or [None]
    sizes = sorted({k[1] for k in groups if k[1] is not None}) or [None]
    corners = [(n, w) for n in dict.fromkeys((ns[0], ns[-1])) for w in dict.fromkeys((sizes[0], sizes[-1]))]
    corners = [c for c in corners if c in groups]
    assert corners, call.id
    per = max(1, 4 // len(corners))
    out = []
    for i, c in enumerate(corners):
        v = groups[c]
        take = min(per, len(v))
        if take == 1:   # corner i takes the i-th variant from the end
            idx = [(len(v) - 1 - i) % len(v)]
        else:
            idx = [len(v) - 1 - k * (len(v) // take) for k in range(take)]
        out += [v[k] for k in idx]
    assert 1 <= len(out) <= 4 and len({p.label for p in out}) == len(out), call.id
    return out


def smallest_and_largest(call, d):
    s = select(call, d)
    return s[0], s[-1]


def device_calls():
    return [c for c in X.CALLS if "device" in c.modes]


# ---- the batch headers' device-mode calls -----------------------------------------------
# Objects of 1, 192 and 193 words and an empty one between them (K = 4 table
# entries), 3 parties, a MAC fault in the last object and a bad character in
# the 192-word one: both verdict arrays are non-trivial.
BSIZES = [1, 0, 192, 193]
BN = 3
B_FAULT = (3, 64)            # (object, local word)
B_BAD = (2, 1, 3, 700)       # (object, party, field, character)
NFB = X.le8(X.NF)


def _verdicts(raw: bytes):
    return [int(v) for v in np.frombuffer(raw, np.int64)]


def _wire_plan(masked):
    from tests import test_wire_batch as WB
    b = WB.Batch(BN, X.PIDS[0], BSIZES, {B_FAULT[0]: [B_FAULT[1]]}, seed=9100)
    o_bad, j, k, off = B_BAD
    texts = WB._with_bad_chars(b, [(o_bad, j, k, off, b"*")])
    bad_at = (5 * j + k) * WB.nchars_of(BSIZES[o_bad]) + off
    toff, nchars = WB.layout(BSIZES, "dense")
    bufs = WB.buffers(texts, BSIZES, toff, nchars)
    K, T = len(BSIZES), sum(BSIZES)
    woff = b.woff
    ins = X.odo_arrs(bufs, X.B64) + [X.Arr("woff", X.OFFS, data=woff), X.Arr("toff", X.OFFS, data=toff)]
    outs = [X.Arr("ff", X.VERDICT, n=8 * K),  # the bad object's entry is unspecified in device mode
            X.Arr("bad", X.VERDICT, verdict=[bad_at if o == o_bad else -1 for o in range(K)])]
    if masked:
        ins.append(X.Arr("secrets", X.WORD, data=b.packed_secrets))
        outs += [X.Arr("o16", X.WORD, n=16 * T), X.Arr("o24", X.REC24, n=24 * T, offset=X.OFFSET[X.WORD])]
    else:
        outs.append(X.Arr("out", X.WORD, n=16 * T))

    def check(whole):
        ff = _verdicts(whole["ff"])
        for o in range(K):
            if o == o_bad:
                continue
            assert ff[o] == (X.NF if b.ff[o] < 0 else b.ff[o]), ("first_fail", o, ff[o])
            lo, hi = int(woff[o]), int(woff[o + 1])
            if masked:
                assert whole["o16"][16 * lo:16 * hi] == b.masked[o].tobytes(), ("masked words", o)
                assert whole["o24"][24 * lo:24 * hi] == b.records[o].tobytes(), ("records", o)
            else:
                assert whole["out"][16 * lo:16 * hi] == b.y[o].tobytes(), ("secrets", o)
    assert b.ff[B_FAULT[0]] == B_FAULT[1]

    def call(L, h, p, fl, s):
        arr = X.b64_struct(p, BN, nchars)
        if masked:
            return L.amph_mask_input_b64_packed(h, arr, BN, p["woff"], p["toff"], K, p["secrets"], p["o16"],
                                                p["o24"], p["ff"], p["bad"], fl, s)
        return L.amph_recombine_verify_b64_packed(h, arr, BN, p["woff"], p["toff"], K, p["out"], p["ff"], p["bad"],
                                                  fl, s)
    return X.Plan("%s_b64_packed K=%d n=%d" % ("mask_input" if masked else "recombine_verify", K, BN), ins, outs,
                  call, check=check)


def _outside_unwritten(g, spans, what):
    keep = np.ones(g.n, bool)
    for a, b in spans:
        keep[a:b] = False
    d = np.nonzero((g.before[g.lo:g.lo + g.n] != g.after[g.lo:g.lo + g.n]) & keep)[0]
    assert d.size == 0, "%s: byte %d outside every object's output changed" % (what, int(d[0]))


def _mask_json_plan():
    from tests import test_upload_batch as UB
    c = UB.MaskCase("big", BN, BSIZES, faults={B_FAULT[0]: B_FAULT[1]}, seed=9200)
    assert UB.FIELDS["big"][0] == X.data(X.PIDS[0]).pr.p
    o_bad, j, k, off = B_BAD
    t = bytearray(c.texts[o_bad][j][k])
    t[off] = ord("*")
    c.texts[o_bad][j][k] = bytes(t)
    bad_at = (5 * j + k) * UB.nchars_of(BSIZES[o_bad]) + off
    toff, bufs = c.slots()
    nchars = len(bufs[0][0])
    K = len(BSIZES)
    ooff, at = [], 32
    for o, W in enumerate(BSIZES):  # output slots with gaps of 16-64 bytes
        ooff.append(at)
        at += -(-UB.data_chars(W) // 16) * 16 + 16 * ((3 * o + 1) % 5)
    cap = at
    ins = X.odo_arrs(bufs, X.B64) + [X.Arr("woff", X.OFFS, data=c.woff), X.Arr("toff", X.OFFS, data=toff),
                                     X.Arr("ooff", X.OFFS, data=np.array(ooff, np.uint64)),
                                     X.Arr("secrets", X.WORD, data=np.ascontiguousarray(np.concatenate(c.secrets)))]
    outs = [X.Arr("text", X.WORD, n=cap), X.Arr("ff", X.VERDICT, n=8 * K),
            X.Arr("bad", X.VERDICT, verdict=[bad_at if o == o_bad else -1 for o in range(K)])]
    live = {}

    def check(whole):
        ff = _verdicts(whole["ff"])
        for o, W in enumerate(BSIZES):
            if o != o_bad:
                assert ff[o] == (X.NF if c.ff[o] < 0 else c.ff[o]), ("first_fail", o, ff[o])
            if c.expect[o] is not None and o != o_bad:
                assert whole["text"][ooff[o]:ooff[o] + UB.data_chars(W)] == c.expect[o], ("text", o)
        _outside_unwritten(live["outs"]["text"], [(ooff[o], ooff[o] + UB.data_chars(W)) for o, W in enumerate(BSIZES)],
                           "out_text")

    def call(L, h, p, fl, s):
        return L.amph_mask_input_json_packed(h, X.b64_struct(p, BN, nchars), BN, p["woff"], p["toff"], K,
                                             p["secrets"], p["text"], cap, p["ooff"], p["ff"], p["bad"], fl, s)
    plan = X.Plan("mask_input_json_packed K=%d n=%d" % (K, BN), ins, outs, call, check=check)
    plan.prepare = lambda i, o: live.update(outs=o)
    return plan


def _convert_json_plan():
    from tests import test_upload_batch as UB
    c = UB.ConvCase("big")
    texts = c.texts(BSIZES)
    o_bad, rec, ch = 2, 5, 3
    at = 1 + 37 * rec + 10 + ch  # '[', whole records, {"value":" , then the record's characters
    t = bytearray(texts[o_bad])
    assert chr(t[at - ch - 1]) == '"' and t[at] != ord("*")
    t[at] = ord("*")
    texts[o_bad] = bytes(t)
    blob, toff = UB.dense(texts)
    wo, K, T = UB.offsets_of(BSIZES), len(BSIZES), sum(BSIZES)
    key = c.key.to_bytes(16, "little")
    ins = [X.Arr("texts", X.JSONTXT, data=blob, offset=5), X.Arr("woff", X.OFFS, data=wo),
           X.Arr("toff", X.OFFS, data=toff), X.Arr("tuples", X.WORD, data=np.ascontiguousarray(c.tup[:T]))]
    outs = [X.Arr("shares", X.WORD, n=32 * T),
            X.Arr("bad", X.VERDICT, verdict=[at if o == o_bad else -1 for o in range(K)])]

    def check(whole):
        for o in range(K):  # a refused text's own rows are unspecified
            lo, hi = int(wo[o]), int(wo[o + 1])
            if o != o_bad:
                assert whole["shares"][32 * lo:32 * hi] == c.share[False][lo:hi].tobytes(), ("share rows", o)

    def call(L, h, p, fl, s):
        return L.amph_convert_share_json_packed(h, p["texts"], len(blob), p["woff"], p["toff"], K, p["tuples"], key,
                                                0, p["shares"], p["bad"], fl, s)
    return X.Plan("convert_share_json_packed K=%d" % K, ins, outs, call, check=check)


def _odo_fields_plan():
    """tests/test_respond_batch.py's own plan with 16-character gaps and two
    rejected objects (11 objects of 0..576 words): the reject words are an
    input, so they arrive with the deferred image -- the header's "behind
    whatever produced the verdicts there", literally."""
    from tests import test_respond_batch as RB
    for plan, before in RB.plans(True):
        if plan.label.endswith("gap=16 reject=True"):
            plan.prepare = lambda i, o, before=before: before.update(
                {name: g.before[g.lo:g.lo + g.n].copy() for name, g in o.items()})
            return plan
    raise AssertionError("the respond batch's plan table has no rejected case")


BATCH_CALLS = [
    ("amph_recombine_verify_b64_packed", lambda: _wire_plan(False)),
    ("amph_mask_input_b64_packed", lambda: _wire_plan(True)),
    ("amph_mask_input_json_packed", _mask_json_plan),
    ("amph_convert_share_json_packed", _convert_json_plan),
    ("amph_odo_fields_b64_packed", _odo_fields_plan),
]
_BATCH_PLANS = {}


def batch_plan(name):
    if name not in _BATCH_PLANS:
        _BATCH_PLANS[name] = dict(BATCH_CALLS)[name]()
    return _BATCH_PLANS[name]
