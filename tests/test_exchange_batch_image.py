"""The exchange batch calls on a context whose host image, small-call arena
and device verdict words another family has just used (capi_batch.hip's
BatchImage, shared by the four many-objects families): after a larger wire
call with a MAC fault and an illegal character -- stale tables, texts and
verdict words in every gap -- the exchange calls give the results they give on
a fresh context, on the arena path and with AMPH_SMALL_BYTES=0 on the staged
one; then the other way round, the wire call after a faulted exchange decode.
The pattern of tests/test_batch_image.py, whose material this reuses."""
import numpy as np
import pytest

from oracle import amphora_oracle as O
from tests import test_batch_image as BI
from tests import test_exchange_batch as XB
from tests.test_wire_batch import check

pytestmark = pytest.mark.gpu

P, R, RINV = O.TEST_PRIME, O.TEST_R, O.TEST_RINV


def wire_call(ctx, m):
    y, ff, bad, st = ctx.recombine_verify_b64_batch(m.texts, m.wire_sizes, status=True)
    assert st[0] == m.wire_status, st
    check(m.wire, dict(y=y, ff=ff, bad=bad), False, bad=m.bad)


def exchange_calls(ctx, per_call):
    mag, neg, dneg, poff, texts = XB.size_case()
    K = len(XB.PAIRS)
    c0 = ctx.exchange_batch_copies()
    got = ctx.exchange_encode_batch([mag[int(poff[o]):int(poff[o + 1])] for o in range(K)],
                                    [neg[int(poff[o]):int(poff[o + 1])] for o in range(K)])
    assert got == list(texts)
    # a decode whose verdict words must all come back clean where the wire call left a fault
    res, bad = ctx.exchange_decode_batch(list(texts), XB.PAIRS)
    assert list(bad) == [-1] * K
    assert np.array_equal(np.concatenate([m for m, _ in res]), mag)
    assert np.array_equal(np.concatenate([g for _, g in res]), dneg)
    # and one with a fault of its own, left behind for the next family
    ftexts, fcounts, fmag, _ = XB.fault_base()
    broken = list(ftexts)
    broken[1] = XB._poke(ftexts[1], 0)
    res, bad, st = ctx.exchange_decode_batch(broken, fcounts, status=True)
    assert st[0] == 3 and [int(x) for x in bad] == [-1, 0, -1, -1], (st, bad)
    assert np.array_equal(res[0][0], fmag[:fcounts[0]]) and np.array_equal(res[3][0], fmag[-fcounts[3]:])
    assert ctx.exchange_batch_copies() - c0 == 3 * per_call


@pytest.mark.parametrize("path", ["arena", "staged"])
def test_exchange_calls_after_another_familys_larger_call(path):
    import amphora_amd as A
    with pytest.MonkeyPatch.context() as mp:
        if path == "staged":
            mp.setenv("AMPH_SMALL_BYTES", "0")
        ctx = A.Context(P, R, RINV)
    large, small = BI.material(len(BI.WIRE), len(BI.CONV)), BI.material(2, 2)
    assert large.bad and large.wire.ff[4] == 192
    per_call = 2 if path == "staged" else 0
    for m in (large, small, large):
        wire_call(ctx, m)
        exchange_calls(ctx, per_call)
    wire_call(ctx, small)  # the wire family takes over the exchange decode's faulted verdict word: all clean
