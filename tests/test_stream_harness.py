"""The deferred runner (tests/stream_cases.py) must be able to fail: torch
stand-ins for a device-mode call on a toy plan, out = in + 1 over 1025 words,
each with one planted error, are rejected with the property that error breaks
named; two correct ones are accepted; and the gate's calibration is checked,
so that nothing passes vacuously.  Torch only: the library is not loaded."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import extent_cases as X  # noqa: E402
from tests import stream_cases as S  # noqa: E402

W = 1025
DATA = ((np.arange(16 * W, dtype=np.int64) * 37 + 11) & 0xFF).astype(np.uint8)


def toy():
    return X.Plan("toy add-one W=%d" % W, [X.Arr("in", X.WORD, data=DATA)],
                  [X.Arr("out", X.WORD, n=16 * W, expect=((DATA.astype(np.int64) + 1) & 0xFF).astype(np.uint8).tobytes())],
                  None)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def gate(torch):
    return S.Gate()


@pytest.fixture(scope="module")
def stream(torch):
    s = torch.cuda.Stream()
    S.run_plan_deferred(toy(), lambda i, o: add_one(torch, i, o), s, None)  # first use of the op, as S2 requires
    return s


def _view(torch, g):
    return g.arena.t[g.start + g.lo: g.start + g.lo + g.n]


def add_one(torch, ins, outs):
    """The op itself, on the current stream, with no temporary."""
    torch.add(_view(torch, ins["in"]), 1, out=_view(torch, outs["out"]))
    return X.OK


def test_the_gate_is_calibrated(gate):
    """Gate() already failed the module if the measured gate lay outside
    [0.5, 5] x the target; measured once more here, on its own."""
    assert gate.target_ms == S.GATE_MS <= S.GATE_CAP_MS and S.GATE_MS >= 10 * S.ENQUEUE_MS
    again = gate.time(gate.cycles)
    print("gate: %d cycles, %.3f ms at calibration, %.3f ms again" % (gate.cycles, gate.measured_ms, again))
    for ms in (gate.measured_ms, again):
        assert 0.5 * S.GATE_MS <= ms <= min(5 * S.GATE_MS, S.GATE_CAP_MS), ms


def test_a_correct_stand_in_is_accepted(torch, gate, stream):
    d = S.run_plan_deferred(toy(), lambda i, o: add_one(torch, i, o), stream, None)  # the ungated warm-up: the
    assert d.status == X.OK                                                          # op's kernel is loaded here
    d = S.run_plan_deferred(toy(), lambda i, o: add_one(torch, i, o), stream, gate)
    assert d.reached is False and d.status == X.OK


def second_stream(torch):
    """Another stream, used once before any gated call: whatever the runtime
    sets up on a stream's first launch (a hardware queue, on the host: calls
    that used a fresh stream have taken 0.3 and 1.0 s) is paid here, as the `stream` fixture pays it
    for the plan's stream, and not inside the window S2 times -- where it also
    let the gate run out before an unchained op was enqueued, so that S1 held."""
    s = torch.cuda.Stream()
    S.run_plan_deferred(toy(), lambda i, o: add_one(torch, i, o), s, None)
    return s


def test_a_helper_stream_chained_by_events_is_accepted(torch, gate, stream):
    helper = second_stream(torch)

    def chained(ins, outs):
        there, back = torch.cuda.Event(), torch.cuda.Event()
        there.record(stream)
        helper.wait_event(there)
        with torch.cuda.stream(helper):
            add_one(torch, ins, outs)
            back.record()
        stream.wait_event(back)
        return X.OK
    d = S.run_plan_deferred(toy(), chained, stream, gate)
    assert d.reached is False


def test_the_default_stream_is_rejected_by_s1(torch, gate, stream):
    """The op reads the zeros and its output is overwritten by the image copy:
    a side stream is not ordered against the null stream on this runtime."""
    def on_default(ins, outs):
        with torch.cuda.stream(torch.cuda.default_stream()):
            return add_one(torch, ins, outs)
    with pytest.raises(AssertionError, match=r"S1 \(order\): toy .*output out differs from the reference"):
        S.run_plan_deferred(toy(), on_default, stream, gate)


def test_an_unchained_second_stream_is_rejected_by_s1(torch, gate, stream):
    other = second_stream(torch)

    def on_other(ins, outs):
        with torch.cuda.stream(other):
            return add_one(torch, ins, outs)
    with pytest.raises(AssertionError, match=r"S1 \(order\): toy .*output out differs from the reference"):
        S.run_plan_deferred(toy(), on_other, stream, gate)
    S.wait_event(_marker(torch, other), "the second stream")


def _marker(torch, s):
    e = torch.cuda.Event()
    e.record(s)
    return e


def test_a_stream_synchronisation_is_rejected_by_s2(torch, gate, stream):
    def waits(ins, outs):
        stream.synchronize()
        return add_one(torch, ins, outs)
    with pytest.raises(AssertionError, match=r"S2 \(no wait\): toy .*the call took [0-9.]+ ms on the host, the gate is"):
        S.run_plan_deferred(toy(), waits, stream, gate)


def test_a_device_wide_wait_is_rejected_by_s2(torch, gate, stream):
    """Freeing device memory for real (the caching allocator's empty_cache)
    waits for the whole device, the gated stream included."""
    def frees(ins, outs):
        big = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
        del big
        torch.cuda.empty_cache()
        return add_one(torch, ins, outs)
    with pytest.raises(AssertionError, match=r"S2 \(no wait\): toy "):
        S.run_plan_deferred(toy(), frees, stream, gate)


def test_a_plan_that_may_wait_is_held_to_s1_only(torch, gate, stream):
    plan = toy()
    plan.label = "base64_decode nbytes=1 offset=0 out_bytes=True"  # a label of the MAY_WAIT dict
    assert S.may_wait(plan.label) and not S.may_wait(toy().label)

    def waits(ins, outs):
        stream.synchronize()
        return add_one(torch, ins, outs)
    S.run_plan_deferred(plan, waits, stream, gate)
    with pytest.raises(AssertionError, match=r"S1 \(order\)"):
        S.run_plan_deferred(plan, lambda i, o: X.OK, stream, gate)  # writes nothing


def test_the_may_wait_dict_cites_the_header():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = open(os.path.join(root, "include", "amphora.h")).read().split("\n")
    assert 1 <= len(S.MAY_WAIT) <= 4
    for pat, why in S.MAY_WAIT.items():
        m = re.match(r"amphora\.h:(\d+)-(\d+) ", why)
        assert m, why
        text = " ".join(lines[int(m.group(1)) - 1:int(m.group(2))])
        assert re.search(r"wait|synchronis", text), (pat, why)
