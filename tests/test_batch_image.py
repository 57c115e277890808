"""The three many-objects families in turn on ONE context (capi_batch.hip's
host image): the wire, upload and respond batch calls share the small-call
arena, the device verdict words and the staged image pair through one
procedure, so each call here runs where another family's call has just left
its bytes -- a larger batch, then a smaller one (the image shrinks in use and
is not reallocated: stale tables, texts and verdict words lie in every gap),
then the larger one again.

Two contexts: the default one, where every call fits the arena, and one
created with AMPH_SMALL_BYTES=0, where the same tiny calls are staged.  Every
output and every verdict entry is checked against the C oracle (wire calls),
the Python oracle (convert, framed mask) or Python's base64 (respond) --
never against another call of the library.  The wire calls carry one object
with a MAC fault and one with an illegal character, so the verdict words are
not all at the sentinel when the next family's call, which must report
all-clean, takes them over.
"""
import base64
import functools

import numpy as np
import pytest

from oracle import amphora_oracle as O
from tests.test_upload_batch import ConvCase, MaskCase
from tests.test_wire_batch import Batch, check, nchars_of

pytestmark = pytest.mark.gpu

P, R, RINV = O.TEST_PRIME, O.TEST_R, O.TEST_RINV
OK, E_VERIFY, E_PARAM = 0, 1, 3
WIRE = [0, 1, 191, 192, 193, 2]  # the wire and respond tile is 192 words
CONV = [0, 1, 127, 128, 129]     # the convert tile is 128 records
FAULT = {4: [192]}               # the 193-word object, the one word of its second tile
BAD_OBJ, BAD_PARTY, BAD_FIELD, BAD_AT = 2, 1, 3, 700  # the 191-word object, party 1's wShares
REJECT = {len(WIRE): 3, 2: 1}    # batch size -> the rejected object of the packed respond call


class Material:
    """Inputs and expected results of one batch size, computed once."""

    def __init__(self, kw, kc):
        self.wire_sizes, self.conv_sizes = WIRE[:kw], CONV[:kc]
        K = kw
        self.wire = Batch(2, "test", self.wire_sizes, {o: f for o, f in FAULT.items() if o < K}, seed=6100)
        self.texts = [[list(p) for p in obj] for obj in self.wire.texts]
        self.bad = {}
        if BAD_OBJ < K:
            t = bytearray(self.texts[BAD_OBJ][BAD_PARTY][BAD_FIELD])
            t[BAD_AT] = ord("*")
            self.texts[BAD_OBJ][BAD_PARTY][BAD_FIELD] = bytes(t)
            self.bad = {BAD_OBJ: (5 * BAD_PARTY + BAD_FIELD) * nchars_of(WIRE[BAD_OBJ]) + BAD_AT}
        self.wire_status = E_PARAM if self.bad else E_VERIFY if any(f >= 0 for f in self.wire.ff) else OK
        self.mask = MaskCase("big", 2, self.wire_sizes, seed=6200)
        self.conv = conv_case()
        self.conv_texts = self.conv.texts(self.conv_sizes)
        self.conv_woff = np.concatenate([[0], np.cumsum(self.conv_sizes)]).astype(int)
        rng = np.random.default_rng(6300 + K)
        T = sum(self.wire_sizes)
        self.fields = rng.integers(0, 256, (5, T, 16), dtype=np.uint8)
        self.fields[1, :3] = 0xFF
        self.fields[2, -2:] = 0x00
        self.fields.setflags(write=False)
        self.woff = np.concatenate([[0], np.cumsum(self.wire_sizes)]).astype(np.uint64)
        self.b64 = [[base64.b64encode(self.fields[k, int(self.woff[o]):int(self.woff[o + 1])].tobytes())
                     for k in range(5)] for o in range(K)]


@functools.lru_cache(maxsize=None)
def conv_case():
    return ConvCase("big")


@functools.lru_cache(maxsize=None)
def material(kw, kc):
    return Material(kw, kc)


def counters(ctx):
    return np.array([ctx.wire_batch_copies(), ctx.upload_batch_copies(), ctx.respond_batch_copies()])


def one_pass(ctx, m, per_call):
    """The six calls in order; per_call = copies of a staged call (0 on the arena path)."""
    K = len(m.wire_sizes)
    moved = []

    def counted(fn, *a, **kw):
        before = counters(ctx)
        res = fn(*a, **kw)
        moved.append(tuple(int(x) for x in counters(ctx) - before))
        return res

    # 1. K_MASK from the wire texts: a MAC fault and an illegal character
    m16, m24, ff, bad, st = counted(ctx.mask_input_b64_batch, m.texts, m.wire_sizes, m.wire.secrets, records=True,
                                    raw=True, status=True)
    assert st[0] == m.wire_status, st
    check(m.wire, dict(m16=m16, m24=m24, ff=ff, bad=bad), True, bad=m.bad)
    # 2. the respond family, no verdicts
    got = counted(ctx.odo_fields_b64_batch, [[np.ascontiguousarray(m.fields[k, int(m.woff[o]):int(m.woff[o + 1])])
                                              for k in range(5)] for o in range(K)])
    assert got == m.b64
    # 3. the convert call takes over the verdict words call 1 left: all clean
    wo = m.conv_woff
    outs, cbad, st = counted(ctx.convert_share_json_batch, m.conv_texts,
                             [np.ascontiguousarray(m.conv.tup[wo[o]:wo[o + 1]]) for o in range(len(m.conv_sizes))],
                             m.conv.key, False, status=True)
    assert st[0] == OK and [int(x) for x in cbad] == [-1] * len(m.conv_sizes), st
    for o, W in enumerate(m.conv_sizes):
        assert outs[o].shape == (W, 32) and np.array_equal(outs[o], m.conv.share[False][wo[o]:wo[o + 1]]), o
    # 4. K_RV on the faulted texts
    y, ff, bad, st = counted(ctx.recombine_verify_b64_batch, m.texts, m.wire_sizes, status=True)
    assert st[0] == m.wire_status, st
    check(m.wire, dict(y=y, ff=ff, bad=bad), False, bad=m.bad)
    # 5. the framed mask call right after: all clean
    texts, ff, bad, st = counted(ctx.mask_input_json_batch, m.mask.texts, m.mask.sizes, m.mask.secrets, status=True)
    assert st[0] == OK and list(ff) == [-1] * K and list(bad) == [-1] * K, st
    assert texts == m.mask.expect
    # 6. the packed respond call with one rejected object, default dense slots
    rj = np.full(K, -1, np.int64)
    rj[REJECT[K]] = 5
    bufs, to = counted(ctx.odo_fields_b64_packed, [np.ascontiguousarray(m.fields[k]) for k in range(5)], m.woff,
                       reject=rj)
    for o in range(K):
        for k in range(5):
            t = bufs[k][int(to[o]):int(to[o]) + nchars_of(m.wire_sizes[o])].tobytes()
            if o == REJECT[K]:
                assert t[:4] == b"!!!!" and len(t) == len(m.b64[o][k]), (o, k)
            else:
                assert t == m.b64[o][k], (o, k)
    c = per_call
    assert moved == [(c, 0, 0), (0, 0, c), (0, c, 0), (c, 0, 0), (0, c, 0), (0, 0, c)]


@pytest.mark.parametrize("path", ["arena", "staged"])
def test_families_in_turn_on_one_context(path):
    import amphora_amd as A
    with pytest.MonkeyPatch.context() as mp:
        if path == "staged":  # no small-call arena: the same tiny calls through the staged image
            mp.setenv("AMPH_SMALL_BYTES", "0")
        ctx = A.Context(P, R, RINV)
    large, small = material(len(WIRE), len(CONV)), material(2, 2)
    assert large.bad and large.wire.ff[4] == 192 and not small.bad
    for m in (large, small, large):
        one_pass(ctx, m, 2 if path == "staged" else 0)
