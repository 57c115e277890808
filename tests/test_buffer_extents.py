"""Every ABI call pinned to its buffers (tests/extent_cases.py): each array of
each entry point of include/amphora.h sits inside guard bands the test owns,
at the least alignment the header allows, with zeros (S0) and then hostile
bytes (S1) around every input.  For every table entry, size and surrounding:

  P1  status, verdict words and outputs equal the reference (the C oracle,
      Python ints, base64 / json -- never another call into the library);
  P2  the bands of every output and verdict word are untouched;
  P3  every input, payload and bands, is unchanged;
  P4  S0 and S1 give the same statuses and outputs.

Device mode runs on the default context and, for the one-word-per-lane
kernels, on one created under AMPH_BLOCK=64 / AMPH_GRID_CAP=3 (192 lanes
stride over 191..400 words: two or more iterations, a partial last wave).
Host mode runs once on the small-call arena path and once through the batched
pipeline with the word count one past a batch boundary.  Sizes are the
smallest at which each structure changes (extent_cases.*_SIZES).
"""
import ctypes as C
import re

import pytest

pytestmark = pytest.mark.gpu

from tests import extent_cases as X  # noqa: E402


class Env:
    def __init__(self, pid):
        import torch
        assert torch.cuda.is_available()
        import amphora_amd as A
        self.pid, self.d = pid, X.data(pid)
        pr = self.d.pr
        self.ctx = A.Context(pr.p, pr.r, pr.rinv)
        with pytest.MonkeyPatch.context() as mp:  # both are read at context creation
            mp.setenv("AMPH_BLOCK", "64")
            mp.setenv("AMPH_GRID_CAP", "3")
            self.strided = A.Context(pr.p, pr.r, pr.rinv)
        with pytest.MonkeyPatch.context() as mp:  # no small-call arena: every host call takes the pipeline
            mp.setenv("AMPH_SMALL_BYTES", "0")
            self.piped = A.Context(pr.p, pr.r, pr.rinv)


_ENVS = {}


def env_of(pid):
    if pid not in _ENVS:
        _ENVS[pid] = Env(pid)
    return _ENVS[pid]


@pytest.fixture(scope="module", autouse=True)
def release_contexts():
    yield
    _ENVS.clear()  # the contexts go with the module, not with the interpreter


def run(ctx, plan, device):
    import torch
    import amphora_amd as A
    L = A._lib.lib
    flags = X.F_DEVICE if device else 0
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream) if device else None

    def invoke(ins, outs):
        p = {k: g.ptr for k, g in list(ins.items()) + list(outs.items())}
        return plan.call(L, ctx._h, p, flags, stream)
    return X.run_plan(plan, device, invoke, torch.cuda.synchronize)


def cases(mode, lane=None):
    """(prime, table entry) pairs; the codecs compute nothing in the field, so
    one prime is every prime for them."""
    out = []
    for pid in X.PIDS:
        for c in X.CALLS:
            if mode not in c.modes or (lane is not None and c.lane != lane):
                continue
            if c.id.startswith(("base64_", "exchange_")) and pid != X.PIDS[0]:
                continue
            out.append(pytest.param(pid, c, id="%s-%s" % (pid, c.id)))
    return out


@pytest.mark.parametrize("pid,call", cases("device"))
def test_device_mode(pid, call):
    env = env_of(pid)
    n = 0
    for plan in call.gen(env.d):
        run(env.ctx, plan, True)
        n += 1
    assert n


@pytest.mark.parametrize("pid,call", cases("device", lane=True))
def test_device_mode_grid_stride(pid, call):
    """64-lane workgroups under a grid cap of 3: the stride loop runs two or
    more iterations and ends in a partial wave."""
    env = env_of(pid)
    for plan in call.gen(env.d, strided=True):
        run(env.strided, plan, True)


@pytest.mark.parametrize("pid,call", cases("host"))
def test_host_mode_small_call(pid, call):
    env = env_of(pid)
    for plan in call.gen(env.d):
        run(env.ctx, plan, False)


def batch_units(plan):
    """The count the host pipeline cuts into batches: words, pairs, or the
    12-byte / 16-character units of the bulk base64 calls."""
    m = re.search(r"\b(W|T|npairs|nbytes)=(\d+)", plan.label)
    if not m:  # a text call (the exchange decode): every case, under a small batch size
        return 129
    return int(m.group(2)) // 12 if m.group(1) == "nbytes" else int(m.group(2))


@pytest.mark.parametrize("pid,call", cases("host"))
def test_host_mode_pipeline(pid, call):
    """AMPH_SMALL_BYTES=0 and a batch of one word fewer than the call has:
    two batches, the second of one word."""
    env = env_of(pid)
    ran = 0
    try:
        for plan in call.gen(env.d):
            u = batch_units(plan)
            if u - 1 not in (7, 64, 128, 129, 192, 255, 256, 1024):
                continue
            env.piped.set_batch_words(u - 1)
            run(env.piped, plan, False)
            ran += 1
    finally:
        env.piped.set_batch_words(4 << 20)
    assert ran
