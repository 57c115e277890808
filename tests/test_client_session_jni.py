"""The client session through the JNI layer (jni/amphora_jni.c's clientBegin /
clientParty / clientFinish* / clientWord / clientFree over
jni/amphora_jni_core.c's amphj_client_*), driven through the mock JNIEnv of
tests/jni_mock (no JDK exists here) against the C oracle: parties handed in
out of order, the three finishes, the failing word and its five sums, a bad
character, and the length checks that fire before the ABI sees a pointer.
"""
import base64
import ctypes as C

import numpy as np
import pytest

from tests.test_jni_core import CLIENT, IAE, Env, F, J, P, R, RINV, jctx, le16  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
IVE = "io/carbynestack/amphora/common/exceptions/IntegrityVerificationException"


def texts_of(odos):
    return [[base64.b64encode(np.ascontiguousarray(f).tobytes()) for f in o] for o in odos]


def begin(e, ctx, W, n):
    h = e.call(CLIENT + "clientBegin", C.c_int64, ctx, C.c_int64(W), C.c_int32(n))
    assert h != 0 and e.exception() is None
    return C.c_int64(h)


def party(e, s, j, five):
    e.call(CLIENT + "clientParty", None, s, C.c_int32(j), *[e.bytes(t) for t in five])


def fed(e, ctx, texts, W, order):
    s = begin(e, ctx, W, len(texts))
    for j in order:
        party(e, s, j, texts[j])
        assert e.exception() is None and e.clean()
    return s


def free(e, s):
    e.call(CLIENT + "clientFree", None, s)


@pytest.mark.parametrize("n,W,order", [(2, 193, (1, 0)), (3, 1000, (2, 0, 1)), (5, 70_000, (4, 1, 3, 0, 2))])
def test_client_session_entry_points(J, jctx, F, n, W, order):  # noqa: F811
    e = Env(J)
    ctx = C.c_int64(jctx)
    odos, _ = F.synth_odos(seed=W + n, n=n, W=W, noncanon_permille=10)
    texts = texts_of(odos)
    oy, _ = F.recombine_verify(odos)
    s = fed(e, ctx, texts, W, order)
    out = e.zeros(16 * W)
    assert e.call(CLIENT + "clientFinishVerify", C.c_int64, s, out) == -1
    assert e.exception() is None and e.clean() and e.read(out) == oy.tobytes()
    free(e, s)
    secrets = F.synth_words(seed=7, count=W - 3, mont=False)
    om, _ = F.mask_input(secrets, [tuple(f[: W - 3] for f in o) for o in odos])
    s = fed(e, ctx, texts, W, order[::-1])
    rec = e.zeros(24 * (W - 3))
    assert e.call(CLIENT + "clientFinishMask", C.c_int64, s, e.bytes(secrets), rec) == -1
    assert e.read(rec) == b"".join(base64.b64encode(w.tobytes()) for w in om) and e.clean()
    free(e, s)
    s = fed(e, ctx, texts, W, order)
    text = e.zeros(37 * (W - 3) + 1)
    assert e.call(CLIENT + "clientFinishMaskJson", C.c_int64, s, e.bytes(secrets), text) == -1
    assert e.read(text) == b"[" + b",".join(b'{"value":"%s"}' % base64.b64encode(w.tobytes()) for w in om) + b"]"
    assert e.clean()
    free(e, s)
    # a MAC fault: the failing word is returned, its five sums are the oracle's recombined values
    fault = W // 3
    bad, _ = F.synth_odos(seed=W + n, n=n, W=W, fault_index=fault)
    s = fed(e, ctx, texts_of(bad), W, order)
    assert e.call(CLIENT + "clientFinishVerify", C.c_int64, s, e.zeros(16 * W)) == fault
    assert e.exception() is None  # a verify failure is returned, the Java side renders the message
    w = e.call(CLIENT + "clientWord", C.c_void_p, s, C.c_int64(fault))
    want = b"".join(F.recombine([o[k][fault:fault + 1] for o in bad]).tobytes() for k in range(5))
    assert e.read(w) == want and e.clean()
    J.mock_clear()
    e.call(CLIENT + "clientWord", C.c_void_p, s, C.c_int64(W))
    assert e.exception()[0] == "java/lang/ArrayIndexOutOfBoundsException"
    free(e, s)
    # more secrets than masks: verified first (a finish with no secrets returns the verdict)
    J.mock_clear()
    s = fed(e, ctx, texts, W, order)
    assert e.call(CLIENT + "clientFinishMask", C.c_int64, s, e.zeros(0), e.zeros(0)) == -1
    assert e.exception() is None
    free(e, s)


def test_region_mode_pins_nothing(J, jctx, F, monkeypatch):  # noqa: F811
    """Above AMPH_JNI_REGION_BYTES (forced to 0 here) the session's entry
    points copy their arrays with Get/SetByteArrayRegion: a party call waits
    for the GPU, and no critical region is open while it does."""
    monkeypatch.setenv("AMPH_JNI_REGION_BYTES", "0")
    e = Env(J)
    ctx = C.c_int64(jctx)
    W, n = 1000, 3
    odos, _ = F.synth_odos(seed=W + n, n=n, W=W)
    texts = texts_of(odos)
    secrets = F.synth_words(seed=7, count=W, mont=False)
    om, _ = F.mask_input(secrets, odos)
    J.mock_clear()
    s = fed(e, ctx, texts, W, (1, 2, 0))
    out = e.zeros(16 * W)
    assert e.call(CLIENT + "clientFinishVerify", C.c_int64, s, out) == -1
    assert e.read(out) == F.recombine_verify(odos)[0].tobytes()
    free(e, s)
    s = fed(e, ctx, texts, W, (0, 2, 1))
    rec = e.zeros(24 * W)
    assert e.call(CLIENT + "clientFinishMask", C.c_int64, s, e.bytes(secrets), rec) == -1
    assert e.read(rec) == b"".join(base64.b64encode(w.tobytes()) for w in om)
    free(e, s)
    assert J.mock_pins() == 0, "a critical region was opened above the threshold"
    assert J.mock_region_copies() > 0 and J.mock_violations() == 0 and J.mock_open_criticals() == 0


def test_bad_character_and_slot_errors(J, jctx, F):  # noqa: F811
    e = Env(J)
    ctx = C.c_int64(jctx)
    W, n = 200, 3
    odos, _ = F.synth_odos(seed=5, n=n, W=W)
    texts = texts_of(odos)
    t = bytearray(texts[1][2])
    t[77] = ord("*")
    texts[1][2] = bytes(t)
    s = begin(e, ctx, W, n)
    party(e, s, 2, texts[2])
    assert e.exception() is None
    J.mock_clear()
    party(e, s, 1, texts[1])
    cls, msg = e.exception()
    assert cls == IAE and "index 77 of party 1's vShares" in msg and e.clean()
    J.mock_clear()
    party(e, s, 2, texts[2])  # a slot twice
    assert e.exception()[0] == IAE and e.clean()
    J.mock_clear()
    e.call(CLIENT + "clientFinishVerify", C.c_int64, s, e.zeros(16 * W))  # a slot missing
    assert e.exception()[0] == IAE and "party 0" in e.exception()[1]
    J.mock_clear()
    party(e, s, 0, texts[0])
    assert e.exception() is None
    J.mock_clear()
    out = e.zeros(16 * W)
    e.call(CLIENT + "clientFinishVerify", C.c_int64, s, out)
    cls, msg2 = e.exception()
    assert cls == IAE and msg2 == msg and e.read(out) == bytes(16 * W) and e.clean()
    free(e, s)


def test_length_checks_fire_before_the_abi(J, jctx, F):  # noqa: F811
    """A Java array shorter than the session's word count implies is rejected
    before libamphora_hip sees its pointer; the session stays usable."""
    e = Env(J)
    ctx = C.c_int64(jctx)
    W, n = 64, 2
    odos, _ = F.synth_odos(seed=6, n=n, W=W)
    texts = texts_of(odos)
    s = begin(e, ctx, W, n)
    J.mock_clear()
    party(e, s, 0, texts[0][:4] + [texts[0][4][:-4]])  # five fields of unequal length
    assert e.exception() == (IAE, "The provided shares must be of the same length") and e.clean()
    J.mock_clear()
    party(e, s, 0, [f[:-4] for f in texts[0]])  # another length than the session's
    assert e.exception()[0] == IAE and "characters, expected" in e.exception()[1] and e.clean()
    J.mock_clear()
    e.call(CLIENT + "clientParty", None, s, C.c_int32(0), *([e.bytes(f) for f in texts[0][:4]] + [None]))
    assert e.exception() == (IAE, "null array") and e.clean()
    J.mock_clear()
    for j in range(n):
        party(e, s, j, texts[j])
    assert e.exception() is None
    J.mock_clear()
    e.call(CLIENT + "clientFinishVerify", C.c_int64, s, e.zeros(16 * W - 1))
    cls, msg = e.exception()
    assert cls == IAE and "the secrets array holds" in msg and e.clean()
    secrets = F.synth_words(seed=7, count=W, mont=False)
    J.mock_clear()
    e.call(CLIENT + "clientFinishMask", C.c_int64, s, e.bytes(secrets), e.zeros(24 * W - 1))
    assert e.exception()[0] == IAE and "the record array holds" in e.exception()[1] and e.clean()
    J.mock_clear()
    e.call(CLIENT + "clientFinishMaskJson", C.c_int64, s, e.bytes(secrets), e.zeros(37 * W))
    assert e.exception()[0] == IAE and "the data array text holds" in e.exception()[1] and e.clean()
    J.mock_clear()
    out = e.zeros(16 * W)  # none of the refusals finished the session
    assert e.call(CLIENT + "clientFinishVerify", C.c_int64, s, out) == -1 and e.exception() is None
    assert e.read(out) == F.recombine_verify(odos)[0].tobytes()
    free(e, s)
    # null sessions and arguments
    for name, rt, args in (("clientParty", None, (C.c_int64(0), C.c_int32(0)) + tuple(e.bytes(b"") for _ in range(5))),
                           ("clientFinishVerify", C.c_int64, (C.c_int64(0), e.zeros(0))),
                           ("clientFinishMask", C.c_int64, (C.c_int64(0), e.zeros(0), e.zeros(0))),
                           ("clientFinishMaskJson", C.c_int64, (C.c_int64(0), e.zeros(0), e.zeros(2))),
                           ("clientWord", C.c_void_p, (C.c_int64(0), C.c_int64(0)))):
        J.mock_clear()
        e.call(CLIENT + name, rt, *args)
        assert e.exception() == (IAE, "null client session") and e.clean(), name
    J.mock_clear()
    assert e.call(CLIENT + "clientBegin", C.c_int64, ctx, C.c_int64(-1), C.c_int32(2)) == 0
    assert e.exception() == (IAE, "negative word count")
    J.mock_clear()
    assert e.call(CLIENT + "clientBegin", C.c_int64, ctx, C.c_int64(4), C.c_int32(17)) == 0
    assert e.exception()[0] == IAE
    e.call(CLIENT + "clientFree", None, C.c_int64(0))
