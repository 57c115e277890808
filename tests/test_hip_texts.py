"""The text matrix: every call of the C ABI that reads base64 (every declaration
with a `bad_char`, `bad_chars` or `bad_index`: the table MATRIX of
tests/text_cases.py, held against the headers by tests/test_text_cases_cpu.py)
on the catalogue of tests/text_cases.py.

The library decides "is this byte in the base64 alphabet" in four independent
implementations.  `test_full_and_latin` holds each of them to all 256 byte
values at every position of its unit (FULL: one offender per call, each call
with its own verdict word of one preallocated array, one synchronisation at
the end) and to every alphabet character at every position (LATIN: the text is
accepted and the outputs are those of the bytes Python's base64 decodes):

* the LDS table: a fast tile of amph_recombine_verify_b64 at 193 words;
* the SWAR classifier with the exact locator behind it: that call's last tile,
  amph_convert_share_json, amph_base64_decode_words, a whole block of
  amph_base64_decode;
* dec6: the last workgroup of amph_base64_decode.

`test_packed_forms` runs EDGE_BYTES x PLACES, PAIRS and ACCEPTED at every size
of TC.SIZES as the objects of ONE call, a clean object after every third case,
in host and device mode; `test_diagonal` runs every other entry of MATRIX over
the diagonal of EDGE_BYTES x PLACES.

Every expected verdict is TC.first_bad's -- the headers' rule in plain Python
-- and every expected output comes from Python's base64 and ``%`` on Python
ints (tests/field_cases.py).  No result is compared with another call of the
library.  Outputs are compared where the headers define them: not for a refused
text, except that a host-mode session writes nothing then (checked on
pre-filled buffers).
"""
import ctypes as C
import functools
import random
from collections import namedtuple

import numpy as np
import pytest

from tests import field_cases as FC
from tests import text_cases as TC
from tests import verdict_cases as VC
from tests.test_hip_primes import NF

pytestmark = pytest.mark.gpu

PID = "test"
OK, E_VERIFY, E_PARAM = 0, 1, 3
F_DEVICE = 1
PREFILL = 0xA5
I64P = C.POINTER(C.c_int64)
WHICH = "diagonal+pairs+accepted"  # what every form outside PACKED_FORMS runs
FINISHES = ["verify", "mask", "mask_json"]
FULL_IMPLS = ["wire_fast", "wire_last", "convert_json", "records", "stream_block", "stream_tail"]
PACKED_FORMS = ["wire_packed", "upload_packed", "convert_packed", "clients"]
DIAGONAL_FORMS = ["stream", "records", "rv_b64", "mask_b64", "mask_json", "convert_json", "wire_batch", "upload_batch",
                  "convert_batch", "client"]
PACKED_MESSAGE = "object %d: %s (%d of %d objects hold an illegal character)"


# ---- plumbing ----------------------------------------------------------------------------
_CTX = {}


def _ctx(pid=PID):
    if pid not in _CTX:
        import torch
        assert torch.cuda.is_available()
        import amphora_amd
        pr = FC.BY_ID[pid]
        _CTX[pid] = amphora_amd.Context(pr.p, pr.r, pr.rinv)
    return _CTX[pid]


def _abi():
    import amphora_amd
    return amphora_amd._lib


@pytest.fixture(scope="module", autouse=True)
def _release():
    """The contexts and the cached device copies end with this module."""
    yield
    import gc
    _CTX.clear()
    pack.cache_clear()
    data_pack.cache_clear()
    gc.collect()


def up(a):
    import torch
    a = np.array(a, copy=True)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


def up_text(t: bytes):
    return up(np.frombuffer(t, np.uint8))


def down(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def verdicts(v):
    """A verdict array of either mode as int64 with -1 for clean."""
    v = np.asarray(v if isinstance(v, np.ndarray) else down(v), np.int64).reshape(-1)
    return np.where(v == NF, -1, v)


def verdict(v):
    if isinstance(v, C.c_int64):
        return v.value
    if isinstance(v, int):
        return v
    return int(verdicts(v)[0])


def i64p(address: int):
    return C.cast(C.c_void_p(address), I64P)


def stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def assert_verdicts(got, want, names, tag):
    got, want = np.asarray(got, np.int64), np.asarray(want, np.int64)
    assert got.shape == want.shape, tag
    off = np.flatnonzero(got != want)
    assert off.size == 0, (tag, "%d of %d verdicts differ" % (off.size, want.size),
                           [(names[i], int(got[i]), int(want[i])) for i in off[:8]])


def rows_on_device(texts):
    """Texts of one length as the rows of one device array, each row 16-byte aligned."""
    n = len(texts[0])
    stride = (n + 15) & ~15
    a = np.full((len(texts), stride), ord("!"), np.uint8)
    a[:, :n] = np.frombuffer(b"".join(texts), np.uint8).reshape(len(texts), n)
    t = up(a)
    assert t.data_ptr() % 16 == 0
    return t, stride


@functools.lru_cache(maxsize=None)
def tuples_and_key(words=TC.RECORDS):
    pr = FC.BY_ID[PID]
    rng = random.Random("text_cases/tuples")
    tuples = [(rng.randrange(pr.p), rng.randrange(pr.p)) for _ in range(words)]
    return tuples, FC.arr([x for t in tuples for x in t], 32), rng.randrange(1, pr.p)


def share_of(words):
    """The party's share of the masked `words` under tuples_and_key, from the Python restatement."""
    tuples, _, key = tuples_and_key()
    out = FC.convert_share(FC.BY_ID[PID], list(words), tuples[:len(words)], key, False)
    return FC.arr([x for pair in out for x in pair], 32)


# ---- expected outputs of a field-text call ---------------------------------------------------------
Outputs = namedtuple("Outputs", "sec y m rec text")


@functools.lru_cache(maxsize=None)
def _outputs(pid, n, W, changed):
    pr = FC.BY_ID[pid]
    b = VC.base(pid, n, W)
    secrets = VC.secrets_for(b)
    y = VC.patched(b.cols[VC.Y], dict(changed))
    masked = FC.mask_words(pr, secrets, y)
    rec = np.frombuffer(b"".join(VC.record(m) for m in masked), np.uint8).reshape(W, 24)
    out = Outputs(FC.arr(secrets), FC.arr(y), FC.arr(masked), rec, VC.data_text(masked))
    for a in out[:4]:
        a.setflags(write=False)
    return out


def outputs(b, e):
    """What an ACCEPTED (or clean) call of the base `b` writes: the secrets used, the recombined
    secrets, the masked words, their records and the framed text."""
    return _outputs(b.pid, b.n, b.W, tuple(sorted((e.changed or {}).items())))


def five_texts(b, case):
    """[party][field] -> the text a case hands in, and the set of edited (party, field)."""
    honest = TC.field_texts(b)
    edited = TC.apply(b, case) if case.edits or case.word_edits else {}
    return [[edited.get((j, k), honest[j][k]) for k in range(5)] for j in range(b.n)], set(edited)


# ---- FULL and LATIN: one decoder implementation each ----------------------------------------------
def count_pairs(cases, positions, impl):
    """The (byte, position of the unit) pairs a case list holds."""
    pairs = set()
    for c in cases:
        for _, _, at, v in c.edits:
            kind = TC.IMPLS[impl].kind
            q = (at - 1) % 37 - 10 if kind == "data" else at % 24 if kind == "record" else at % 16
            pairs.add((v, q))
    assert all(0 <= q < positions for _, q in pairs)
    return len(pairs)


def wire_call(lib, ctx, b, honest_rows, stride, edited_at, out, ffp, badp, sp):
    """amph_recombine_verify_b64 in device mode: the honest rows, with the fields of
    `edited_at` {(party, field): address} in their place."""
    A = _abi()
    arr = (A._AmphOdoB64 * b.n)()
    for j in range(b.n):
        ptrs = [edited_at.get((j, k), honest_rows + (5 * j + k) * stride) for k in range(5)]
        arr[j] = A._AmphOdoB64(*ptrs, TC.wire_chars(b.W))
    st = lib.amph_recombine_verify_b64(ctx._h, arr, b.n, b.W, out, ffp, badp, F_DEVICE, sp)
    assert st == OK, (st, lib.amph_last_error())
    return arr


def run_full_wire(impl, n):
    import torch
    ctx, lib = _ctx(), _abi().lib
    b = VC.base(PID, n, TC.W_FULL)
    W, positions = b.W, TC.IMPLS[impl].positions
    honest, stride = rows_on_device([t for o in TC.field_texts(b) for t in o])
    sp = stream_ptr()
    # FULL: 256 x 16 calls, one offender each
    cases = TC.full_cases(impl, n)
    TC.self_check(b, cases)
    assert len(cases) == count_pairs(cases, positions, impl) == 256 * positions
    applied = [next(iter(TC.apply(b, c).items())) for c in cases]
    rows, stride2 = rows_on_device([t for _, t in applied])
    assert stride2 == stride
    N = len(cases)
    bad = torch.zeros(N, dtype=torch.int64, device="cuda")
    ff = torch.zeros(N, dtype=torch.int64, device="cuda")
    out = torch.empty((W, 16), dtype=torch.uint8, device="cuda")
    keep = [wire_call(lib, ctx, b, honest.data_ptr(), stride, {jk: rows.data_ptr() + i * stride}, out.data_ptr(),
                      i64p(ff.data_ptr() + 8 * i), i64p(bad.data_ptr() + 8 * i), sp)
            for i, (jk, _) in enumerate(applied)]
    assert_verdicts(verdicts(bad), [c.want for c in cases], [c.name for c in cases], (impl, n, "FULL"))
    # LATIN: accepted, and the outputs are those of the decoded words
    latin = TC.latin_cases(impl, n)
    assert count_pairs(latin, positions, impl) == 64 * positions
    expects = [TC.expect(b, c) for c in latin]
    applied = [next(iter(TC.apply(b, c).items())) for c in latin]
    rows, _ = rows_on_device([t for _, t in applied])
    L = len(latin)
    bad = torch.zeros(L, dtype=torch.int64, device="cuda")
    ff = torch.zeros(L, dtype=torch.int64, device="cuda")
    outs = torch.empty((L, W, 16), dtype=torch.uint8, device="cuda")
    keep += [wire_call(lib, ctx, b, honest.data_ptr(), stride, {jk: rows.data_ptr() + i * stride},
                       outs[i].data_ptr(), i64p(ff.data_ptr() + 8 * i), i64p(bad.data_ptr() + 8 * i), sp)
             for i, (jk, _) in enumerate(applied)]
    names = [c.name for c in latin]
    assert_verdicts(verdicts(bad), [-1] * L, names, (impl, n, "LATIN bad_char"))
    assert all(e.bad == -1 and e.ff >= 0 for e in expects) and any(e.changed for e in expects)
    assert_verdicts(verdicts(ff), [e.ff for e in expects], names, (impl, n, "LATIN first_fail"))
    got = down(outs)
    for i, e in enumerate(expects):
        assert np.array_equal(got[i], outputs(b, e).y), (impl, n, names[i])
    print("%s n=%d: FULL %d, LATIN %d (byte, position) pairs" % (impl, n, N, 64 * positions))


def single_call(impl_or_kind):
    """-> call(ctx, text address, out address, verdict address, stream) for a single-text kind."""
    lib = _abi().lib
    kind = TC.IMPLS[impl_or_kind].kind if impl_or_kind in TC.IMPLS else impl_or_kind
    _, tup, key = tuples_and_key()
    if kind == "data":
        dtup, n = up(tup), len(TC.single_text("data"))
        return lambda ctx, t, out, badp, sp: lib.amph_convert_share_json(
            ctx._h, t, n, TC.RECORDS, dtup.data_ptr(), key.to_bytes(16, "little"), 0, out, badp, F_DEVICE, sp)
    if kind == "record":
        return lambda ctx, t, out, badp, sp: lib.amph_base64_decode_words(ctx._h, t, TC.RECORDS, out, badp, F_DEVICE, sp)
    n = len(TC.single_text("stream"))
    return lambda ctx, t, out, badp, sp: lib.amph_base64_decode(ctx._h, t, n, out, None, badp, F_DEVICE, sp)


def single_output(kind, text):
    """The bytes an accepted single text gives."""
    raw = TC.decoded(text, kind)
    if kind == "data":
        return share_of(TC.words_of(raw)).reshape(-1)
    return np.frombuffer(raw, np.uint8)


def run_full_single(impl):
    import torch
    ctx = _ctx()
    kind, positions = TC.IMPLS[impl].kind, TC.IMPLS[impl].positions
    text = TC.single_text(kind)
    call = single_call(impl)
    sp = stream_ptr()
    out_bytes = {"data": 32 * TC.RECORDS, "record": 16 * TC.RECORDS, "stream": 3 * len(text) // 4}[kind]
    cases = TC.full_cases(impl)
    TC.single_self_check(kind, cases)
    assert len(cases) == count_pairs(cases, positions, impl) == 256 * positions
    rows, stride = rows_on_device([TC.edited_single(text, c) for c in cases])
    N = len(cases)
    bad = torch.zeros(N, dtype=torch.int64, device="cuda")
    out = torch.empty(out_bytes + 16, dtype=torch.uint8, device="cuda")
    for i in range(N):
        st = call(ctx, rows.data_ptr() + i * stride, out.data_ptr(), i64p(bad.data_ptr() + 8 * i), sp)
        assert st == OK, (impl, i, st)
    assert_verdicts(verdicts(bad), [TC.verdict_of(kind, c.want) for c in cases], [c.name for c in cases], (impl, "FULL"))
    latin = TC.latin_texts(impl, text)
    assert len({(row[q], q) for _, row in TC.latin_rows(impl) for q in range(positions)}) == 64 * positions
    assert all(t != text and len(t) == len(text) for t in latin)
    want = [single_output(kind, t) for t in latin]
    rows, stride = rows_on_device(latin)
    L = len(latin)
    bad = torch.zeros(L, dtype=torch.int64, device="cuda")
    outs = torch.full((L, (out_bytes + 31) & ~15), PREFILL, dtype=torch.uint8, device="cuda")
    for i in range(L):
        assert call(ctx, rows.data_ptr() + i * stride, outs[i].data_ptr(), i64p(bad.data_ptr() + 8 * i), sp) == OK
    assert_verdicts(verdicts(bad), [-1] * L, list(range(L)), (impl, "LATIN"))
    got = down(outs)
    for i in range(L):
        assert np.array_equal(got[i, :len(want[i])], want[i]), (impl, "LATIN", i)
    print("%s: FULL %d, LATIN %d (byte, position) pairs" % (impl, N, 64 * positions))


@pytest.mark.parametrize("n", TC.PARTIES)
@pytest.mark.parametrize("impl", ["wire_fast", "wire_last"])
def test_full_and_latin_wire(impl, n):
    run_full_wire(impl, n)


@pytest.mark.parametrize("impl", ["convert_json", "records", "stream_block", "stream_tail"])
def test_full_and_latin(impl):
    run_full_single(impl)


# ---- the many-objects forms: object o carries case o ---------------------------------------------
class Pack:
    """TC.packed_objects(PID, n, which) in the arrays the packed calls take and give."""

    def __init__(self, n, which):
        P = self.P = TC.packed_objects(PID, n, which)
        self.n, self.K = n, len(P.objects)
        self.names = [o.name for o in P.objects]
        self.sizes = list(P.sizes)
        self.woff = np.asarray(P.woff, np.uint64)
        self.foff = np.asarray(P.foff, np.uint64)
        pieces = [[[] for _ in range(5)] for _ in range(n)]
        self.texts, self.bad, self.ff, self.by_party, outs = [], [], [], [], []
        for o in P.objects:
            b = o.base
            five, edited = five_texts(b, o.case)
            gap = b"!" * (VC.wire_slot_chars(b.W) - TC.wire_chars(b.W))
            for j in range(n):
                for k in range(5):
                    pieces[j][k] += [five[j][k], gap]
            self.texts.append(five)
            self.bad.append(o.expect.bad)
            self.ff.append(o.expect.ff)
            self.by_party.append(TC.by_party(b, o.case) if edited else [-1] * n)
            outs.append(outputs(b, o.expect))
        self.outs = outs
        self.bufs = [[np.frombuffer(b"".join(pieces[j][k]), np.uint8) for k in range(5)] for j in range(n)]
        assert all(f.size == P.field_chars for five in self.bufs for f in five)
        self.sec, self.y, self.m, self.rec = (np.concatenate([getattr(x, f) for x in outs])
                                              for f in ("sec", "y", "m", "rec"))
        self.accepted = np.asarray(self.bad) < 0
        self.ok_words = np.repeat(self.accepted, self.sizes)
        refused = np.flatnonzero(~self.accepted)
        assert refused.size and self.accepted.sum() >= self.K // 5
        first = int(refused[0])
        self.message = PACKED_MESSAGE % (first, _abi().wire_bad_char_message(self.bad[first], self.sizes[first]),
                                         refused.size, self.K)
        self._dev = None

    def device(self):
        if self._dev is None:
            self._dev = ([[up(f) for f in five] for five in self.bufs], up(self.woff), up(self.foff), up(self.sec))
        return self._dev

    def check(self, ff, bad, on_dev, tag):
        """bad_char whole; first_fail where the headers define it: on every accepted object, and
        -1 on a refused one in host mode (amphora_wire_batch.h)."""
        assert_verdicts(verdicts(bad), self.bad, self.names, (tag, "bad_char"))
        ff = verdicts(ff)
        want = np.asarray([-1 if f is None else f for f in self.ff])
        at = np.arange(self.K) if not on_dev else np.flatnonzero(self.accepted)
        assert_verdicts(ff[at], want[at], [self.names[i] for i in at], (tag, "first_fail"))

    def check_words(self, got, want, tag):
        got = got if isinstance(got, np.ndarray) else down(got)
        assert got.shape == want.shape and np.array_equal(got[self.ok_words], want[self.ok_words]), tag

    def check_uploads(self, text, offsets, tag):
        text = text if isinstance(text, np.ndarray) else down(text)
        offsets = [int(x) for x in (offsets if isinstance(offsets, np.ndarray) else down(offsets))]
        dense = np.concatenate([[0], np.cumsum([VC.upload_slot_chars(W) for W in self.sizes])])[:self.K]
        assert offsets == dense.tolist(), tag
        for o in np.flatnonzero(self.accepted):
            want = self.outs[o].text
            assert text[offsets[o]:offsets[o] + len(want)].tobytes() == want, (tag, self.names[o])


@functools.lru_cache(maxsize=2)
def pack(n, which="edge+pairs+accepted"):
    return Pack(n, which)


def modes(M):
    """(on_dev, buffers, word offsets, text offsets, secrets) of host and device mode."""
    return [(False, M.bufs, M.woff, M.foff, M.sec), (True,) + M.device()]


def run_wire_packed(n):
    ctx, M = _ctx(), pack(n)
    for on_dev, tx, wo, to, sec in modes(M):
        want_status = (OK, "") if on_dev else (E_PARAM, M.message)
        y, ff, bad, status = ctx.recombine_verify_b64_packed(tx, wo, to, status=True)
        assert status == want_status, (on_dev, status)
        M.check(ff, bad, on_dev, ("rv", on_dev))
        M.check_words(y, M.y, ("rv", on_dev))
        m16, rec, ff, bad, status = ctx.mask_input_b64_packed(tx, wo, to, sec, records=True, raw=True, status=True)
        assert status == want_status, (on_dev, status)
        M.check(ff, bad, on_dev, ("mask", on_dev))
        M.check_words(m16, M.m, ("mask", on_dev))
        M.check_words(rec, M.rec, ("records", on_dev))


def run_upload_packed(n):
    ctx, M = _ctx(), pack(n)
    for on_dev, tx, wo, to, sec in modes(M):
        text, oo, ff, bad, status = ctx.mask_input_json_packed(tx, wo, to, sec, status=True)
        assert status == ((OK, "") if on_dev else (E_PARAM, M.message)), (on_dev, status)
        M.check(ff, bad, on_dev, ("json", on_dev))
        M.check_uploads(text, oo, ("json", on_dev))


def arrival(n):
    """2, 0, 1 (then the rest in order); a single party as it is."""
    return [j for j in (2, 0, 1) if j < n] + list(range(3, n))


def run_clients(n):
    """The K-secret session: each party's call reports that party's offenders per object, the
    finish the minimum over the parties; the other objects' outputs are written in both modes."""
    ctx, M = _ctx(), pack(n)
    order = arrival(n)
    for on_dev, tx, _, _, sec in modes(M):
        for finish in FINISHES:
            tag = (finish, on_dev)
            with (ctx.clients_begin_dev(M.woff, n) if on_dev else ctx.clients_begin(M.woff, n)) as s:
                assert s.field_offsets.tolist() == M.foff.tolist(), tag
                parts = []
                for j in order:
                    want = [v[j] for v in M.by_party]
                    if on_dev:
                        parts.append((j, want, s.party(j, tx[j])))
                    else:
                        got, (st, _) = s.party(j, tx[j], status=True)
                        assert st == (E_PARAM if max(want) >= 0 else OK), (tag, j, st)
                        assert_verdicts(verdicts(got), want, M.names, (tag, "party", j))
                if finish == "verify":
                    y, ff, bad, status = s.finish_verify(status=True)
                elif finish == "mask":
                    m16, rec, ff, bad, status = s.finish_mask(sec, records=True, raw=True, status=True)
                else:
                    text, ff, bad, status = s.finish_mask_json(sec, status=True)
                assert status == ((OK, "") if on_dev else (E_PARAM, M.message)), (tag, status)
                for j, want, got in parts:
                    assert_verdicts(verdicts(got), want, M.names, (tag, "party", j))
                M.check(ff, bad, on_dev, tag)
                if finish == "verify":
                    M.check_words(y, M.y, tag)
                elif finish == "mask":
                    M.check_words(m16, M.m, tag)
                    M.check_words(rec, M.rec, tag)
                else:
                    M.check_uploads(text, s.upload_offsets, tag)


class DataPack:
    """"data" array texts of 129 records as the objects of one convert call: every case of
    `cases`, a clean text after every third, and the LATIN text (accepted, another share)."""

    def __init__(self, diagonal):
        text = TC.single_text("data")
        cases = (TC.single_diagonal("data") if diagonal else TC.single_edge_cases("data")) + TC.single_pairs("data")
        TC.single_self_check("data", cases)
        latin, = TC.latin_texts("convert_json", text)
        honest_share, latin_share = share_of(TC.record_words()), single_output("data", latin).reshape(-1, 32)
        assert not np.array_equal(honest_share, latin_share)
        self.names, self.texts, self.bad, shares = [], [], [], []
        for q, c in enumerate(cases):
            self.names.append(c.name)
            self.texts.append(TC.edited_single(text, c))
            self.bad.append(c.want)
            shares.append(honest_share)
            if q % 3 == 2:
                self.names.append("clean%d" % q)
                self.texts.append(text)
                self.bad.append(-1)
                shares.append(honest_share)
        self.names.append("latin")
        self.texts.append(latin)
        self.bad.append(-1)
        shares.append(latin_share)
        self.K = len(self.texts)
        dense = b"".join(self.texts)  # the dense concatenation: any alignment; whole 16-byte granules
        self.buf = np.frombuffer(dense + b"!" * (-len(dense) % 16), np.uint8)
        self.toff = (np.arange(self.K) * len(text)).astype(np.uint64)
        self.woff = (np.arange(self.K + 1) * TC.RECORDS).astype(np.uint64)
        _, tup, self.key = tuples_and_key()
        self.tuples = np.tile(tup, (self.K, 1))
        self.share = np.concatenate(shares)
        self.shares = shares
        self.ok_words = np.repeat(np.asarray(self.bad) < 0, TC.RECORDS)
        refused = np.flatnonzero(np.asarray(self.bad) >= 0)
        self.message = "object %d: Malformed MaskedInput data text at offset %d (" % (refused[0], self.bad[refused[0]])
        self.count = "%d of %d texts refused)" % (refused.size, self.K)

    def check_status(self, status, on_dev):
        if on_dev:
            assert status == (OK, ""), status
        else:
            assert status[0] == E_PARAM and status[1].startswith(self.message) and status[1].endswith(self.count), status


@functools.lru_cache(maxsize=None)
def data_pack(diagonal):
    return DataPack(diagonal)


def run_convert_packed(n):
    ctx, D = _ctx(), data_pack(False)
    for on_dev in (False, True):
        args = (up(D.buf), up(D.woff), up(D.toff), up(D.tuples)) if on_dev else (D.buf, D.woff, D.toff, D.tuples)
        out, bad, status = ctx.convert_share_json_packed(*args, D.key, False, status=True)
        D.check_status(status, on_dev)
        assert_verdicts(verdicts(bad), D.bad, D.names, ("convert_packed", on_dev))
        out = down(out) if on_dev else out
        assert out.shape == D.share.shape and np.array_equal(out[D.ok_words], D.share[D.ok_words]), on_dev


RUN_PACKED = {"wire_packed": run_wire_packed, "upload_packed": run_upload_packed, "convert_packed": run_convert_packed,
              "clients": run_clients}
assert list(RUN_PACKED) == PACKED_FORMS == list(TC.PACKED_FORMS)


def packed_parameters():
    """Every packed form at every party count; the convert call has no parties."""
    return [(form, n) for n in TC.PARTIES for form in PACKED_FORMS if form != "convert_packed" or n == 1]


@pytest.mark.parametrize("form,n", packed_parameters())
def test_packed_forms(form, n):
    RUN_PACKED[form](n)


# ---- every other entry of the matrix: the diagonal -------------------------------------------------
def host_wire_call(form, ctx, five, W, sec):
    """The single wire-text call `form` in host mode through the C ABI, on pre-filled outputs:
    -> (status, first_fail, bad_char, outputs, message)."""
    lib = _abi().lib
    arr, keep = ctx._text_structs(five)
    ff, bad = C.c_int64(-7), C.c_int64(-7)
    if form == "rv_b64":
        outs = [np.full((W, 16), PREFILL, np.uint8)]
        st = lib.amph_recombine_verify_b64(ctx._h, arr, len(five), W, outs[0].ctypes.data, C.byref(ff), C.byref(bad), 0,
                                           None)
    elif form == "mask_b64":
        outs = [np.full((W, 16), PREFILL, np.uint8), np.full((W, 24), PREFILL, np.uint8)]
        st = lib.amph_mask_input_b64(ctx._h, arr, len(five), W, sec.ctypes.data, W, outs[0].ctypes.data,
                                     outs[1].ctypes.data, C.byref(ff), C.byref(bad), 0, None)
    else:
        cap = 37 * W + 1
        outs = [np.full(cap, PREFILL, np.uint8)]
        st = lib.amph_mask_input_json(ctx._h, arr, len(five), W, sec.ctypes.data, W, outs[0].ctypes.data, cap,
                                      C.byref(ff), C.byref(bad), 0, None)
    return st, ff.value, bad.value, outs, (lib.amph_last_error().decode() if st else "")


def wanted(form, R):
    if form in ("rv_b64", "verify"):
        return [R.y]
    if form in ("mask_b64", "mask"):
        return [R.m, R.rec]
    return [np.frombuffer(R.text, np.uint8)]


def run_single_wire(form, n, pid=PID, which=WHICH):
    """amph_recombine_verify_b64 / amph_mask_input_b64 / amph_mask_input_json at every size."""
    ctx, A = _ctx(pid), _abi()
    for W in TC.SIZES:
        b, cs = TC.catalogue(pid, n, W, which)
        dev_honest = [[up_text(t) for t in o] for o in TC.field_texts(b)]
        dsec = up(outputs(b, TC.Expect(-1, -1, {})).sec)
        pending = []
        for c, e in cs:
            tag = (form, n, W, c.name)
            five, edited = five_texts(b, c)
            R = outputs(b, e)
            st, ff, bad, outs, msg = host_wire_call(form, ctx, five, W, R.sec)
            if e.bad >= 0:
                assert (st, bad, msg) == (E_PARAM, e.bad, A.wire_bad_char_message(e.bad, W)), (tag, st, bad, msg)
            else:
                assert (st, ff, bad) == (E_VERIFY if e.ff >= 0 else OK, e.ff, -1), (tag, st, ff, bad)
                for g, w in zip(outs, wanted(form, R)):
                    assert g.shape == w.shape and np.array_equal(g, w), tag
            dtx = [[up_text(five[j][k]) if (j, k) in edited else dev_honest[j][k] for k in range(5)] for j in range(n)]
            if form == "rv_b64":
                *outs, ff, bad = ctx.recombine_verify_b64(dtx, W)
            elif form == "mask_b64":
                *outs, ff, bad = ctx.mask_input_b64(dtx, W, dsec, records=True, raw=True)
            else:
                *outs, ff, bad = ctx.mask_input_json(dtx, W, dsec)
            pending.append((tag, e, R, outs, ff, bad))
        for tag, e, R, outs, ff, bad in pending:
            assert verdict(bad) == e.bad, (tag, "device", verdict(bad), e.bad)
            if e.bad < 0:
                assert verdict(ff) == e.ff, (tag, "device", verdict(ff), e.ff)
                for g, w in zip(outs, wanted(form, R)):
                    assert np.array_equal(down(g).reshape(w.shape), w), (tag, "device")


def run_client(n):
    """The client session: the offending party's call reports its verdict and the others stay
    clean, each of the three finishes repeats the session's verdict, a host-mode finish leaves
    its pre-filled outputs alone on either error; the parties arrive 2, 0, 1."""
    ctx, A = _ctx(), _abi()
    lib = A.lib
    order = arrival(n)
    for W in TC.SIZES:
        b, cs = TC.catalogue(PID, n, W, WHICH)
        dev_honest = [[up_text(t) for t in o] for o in TC.field_texts(b)]
        clean = outputs(b, TC.Expect(-1, -1, {}))
        dsec = up(clean.sec)
        pending = []
        for c, e in cs:
            five, edited = five_texts(b, c)
            dtx = [[up_text(five[j][k]) if (j, k) in edited else dev_honest[j][k] for k in range(5)] for j in range(n)]
            per_party = TC.by_party(b, c)
            assert min([v for v in per_party if v >= 0], default=-1) == e.bad
            R = outputs(b, e)
            for finish in FINISHES:
                tag = ("client", finish, n, W, c.name)
                s = ctx.client_begin(W, n)
                try:
                    for j in order:
                        arr, keep = ctx._text_structs([five[j]])
                        v = C.c_int64(-7)
                        st = lib.amph_client_party(s._h, j, arr, C.byref(v))
                        assert (st, v.value) == ((E_PARAM, per_party[j]) if per_party[j] >= 0 else (OK, -1)), (tag, j)
                        if st:
                            assert lib.amph_last_error().decode() == A.wire_bad_char_message(per_party[j], W), (tag, j)
                    ff, bad = C.c_int64(-7), C.c_int64(-7)
                    if finish == "verify":
                        outs = [np.full((W, 16), PREFILL, np.uint8)]
                        st = lib.amph_client_finish_verify(s._h, outs[0].ctypes.data, C.byref(ff), C.byref(bad))
                    elif finish == "mask":
                        outs = [np.full((W, 16), PREFILL, np.uint8), np.full((W, 24), PREFILL, np.uint8)]
                        st = lib.amph_client_finish_mask(s._h, R.sec.ctypes.data, W, outs[0].ctypes.data,
                                                         outs[1].ctypes.data, C.byref(ff), C.byref(bad))
                    else:
                        cap = 37 * W + 1
                        outs = [np.full(cap, PREFILL, np.uint8)]
                        st = lib.amph_client_finish_mask_json(s._h, R.sec.ctypes.data, W, outs[0].ctypes.data, cap,
                                                              C.byref(ff), C.byref(bad))
                    if e.bad >= 0:
                        assert (st, bad.value) == (E_PARAM, e.bad), (tag, st, bad.value)
                        assert lib.amph_last_error().decode() == A.wire_bad_char_message(e.bad, W), tag
                    else:
                        assert (st, ff.value, bad.value) == (E_VERIFY if e.ff >= 0 else OK, e.ff, -1), (tag, st)
                    for g, w in zip(outs, wanted(finish, R)):
                        if st:
                            assert (g == PREFILL).all(), tag  # host mode writes no output on either error
                        else:
                            assert g.shape == w.shape and np.array_equal(g, w), tag
                finally:
                    s.close()
                s = ctx.client_begin_dev(W, n)
                try:
                    parts = [(j, s.party(j, dtx[j])) for j in order]
                    if finish == "verify":
                        *outs, ff, bad = s.finish_verify()
                    elif finish == "mask":
                        *outs, ff, bad = s.finish_mask(dsec, records=True, raw=True)
                    else:
                        *outs, ff, bad = s.finish_mask_json(dsec)
                finally:
                    s.close()
                pending.append((tag, e, R, per_party, parts, outs, ff, bad, finish))
        for tag, e, R, per_party, parts, outs, ff, bad, finish in pending:
            assert [verdict(v) for _, v in parts] == [per_party[j] for j, _ in parts], (tag, "device")
            assert verdict(bad) == e.bad, (tag, "device", verdict(bad), e.bad)
            if e.bad < 0:
                assert verdict(ff) == e.ff, (tag, "device")
                for g, w in zip(outs, wanted(finish, R)):
                    assert np.array_equal(down(g).reshape(w.shape), w), (tag, "device")


def run_wire_batch(n):
    """The gather forms of the wire-text calls: host memory only."""
    ctx, M = _ctx(), pack(n, WHICH)
    ys, ff, bad, status = ctx.recombine_verify_b64_batch(M.texts, M.sizes, status=True)
    assert status == (E_PARAM, M.message), status
    M.check(ff, bad, False, "rv_batch")
    M.check_words(np.concatenate(ys), M.y, "rv_batch")
    m16, rec, ff, bad, status = ctx.mask_input_b64_batch(M.texts, M.sizes, [x.sec for x in M.outs], records=True, raw=True,
                                                         status=True)
    assert status == (E_PARAM, M.message), status
    M.check(ff, bad, False, "mask_batch")
    M.check_words(np.concatenate(m16), M.m, "mask_batch")
    M.check_words(np.concatenate(rec), M.rec, "mask_batch")


def run_upload_batch(n):
    ctx, M = _ctx(), pack(n, WHICH)
    texts, ff, bad, status = ctx.mask_input_json_batch(M.texts, M.sizes, [x.sec for x in M.outs], status=True)
    assert status == (E_PARAM, M.message), status
    M.check(ff, bad, False, "json_batch")
    for o in np.flatnonzero(M.accepted):
        assert texts[o] == M.outs[o].text, M.names[o]


def run_convert_batch(n):
    ctx, D = _ctx(), data_pack(True)
    _, tup, key = tuples_and_key()
    outs, bad, status = ctx.convert_share_json_batch(D.texts, [tup] * D.K, key, False, status=True)
    D.check_status(status, False)
    assert_verdicts(verdicts(bad), D.bad, D.names, "convert_batch")
    for o in range(D.K):
        if D.bad[o] < 0:
            assert np.array_equal(outs[o], D.shares[o]), D.names[o]


def run_single_text(form, n):
    """amph_base64_decode, amph_base64_decode_words, amph_convert_share_json: the status, the
    verdict and the message in host mode, the verdict word in device mode."""
    import torch
    ctx, lib = _ctx(), _abi().lib
    kind = {"stream": "stream", "records": "record", "convert_json": "data"}[form]
    text = TC.single_text(kind)
    cases = TC.single_diagonal(kind) + TC.single_pairs(kind)
    TC.single_self_check(kind, cases)
    _, tup, key = tuples_and_key()
    out = np.empty(32 * TC.RECORDS + len(text), np.uint8)
    message = {"stream": "Illegal base64 character at index %d", "records": "Illegal base64 word record at index %d",
               "convert_json": "Malformed MaskedInput data text at offset %d ("}[form]
    for c in cases:
        t = TC.edited_single(text, c)
        want = TC.verdict_of(kind, c.want)
        bad = C.c_int64(-7)
        if form == "stream":
            ob = C.c_size_t(0)
            st = lib.amph_base64_decode(ctx._h, t, len(t), out.ctypes.data, C.byref(ob), C.byref(bad), 0, None)
        elif form == "records":
            st = lib.amph_base64_decode_words(ctx._h, t, TC.RECORDS, out.ctypes.data, C.byref(bad), 0, None)
        else:
            st = lib.amph_convert_share_json(ctx._h, t, len(t), TC.RECORDS, tup.ctypes.data, key.to_bytes(16, "little"), 0,
                                             out.ctypes.data, C.byref(bad), 0, None)
        msg = lib.amph_last_error().decode()
        assert (st, bad.value) == (E_PARAM, want) and msg.startswith(message % want), (form, c.name, st, bad.value, msg)
        assert form == "convert_json" or msg == message % want, (form, c.name, msg)
    call, sp = single_call(kind), stream_ptr()
    rows, stride = rows_on_device([TC.edited_single(text, c) for c in cases] + [text])
    N = len(cases) + 1
    bad = torch.zeros(N, dtype=torch.int64, device="cuda")
    dout = torch.empty(out.size, dtype=torch.uint8, device="cuda")
    for i in range(N):
        assert call(ctx, rows.data_ptr() + i * stride, dout.data_ptr(), i64p(bad.data_ptr() + 8 * i), sp) == OK
    assert_verdicts(verdicts(bad), [TC.verdict_of(kind, c.want) for c in cases] + [-1], [c.name for c in cases] + ["honest"],
                    (form, "device"))
    want = single_output(kind, text)  # the honest text, last: accepted, and decoded as Python decodes it
    assert np.array_equal(down(dout)[:len(want)], want), form


RUN = {"stream": functools.partial(run_single_text, "stream"), "records": functools.partial(run_single_text, "records"),
       "convert_json": functools.partial(run_single_text, "convert_json"),
       "rv_b64": functools.partial(run_single_wire, "rv_b64"), "mask_b64": functools.partial(run_single_wire, "mask_b64"),
       "mask_json": functools.partial(run_single_wire, "mask_json"), "wire_batch": run_wire_batch,
       "upload_batch": run_upload_batch, "convert_batch": run_convert_batch, "client": run_client}
assert set(RUN) == set(DIAGONAL_FORMS) and not set(RUN) & set(RUN_PACKED)
assert set(RUN) | set(RUN_PACKED) == {e.form for e in TC.MATRIX.values()}
NO_PARTIES = ("stream", "records", "convert_json", "convert_batch")


def diagonal_parameters():
    return [(form, n) for form in DIAGONAL_FORMS for n in (TC.PARTIES if form not in NO_PARTIES else (1,))]


@pytest.mark.parametrize("form,n", diagonal_parameters())
def test_diagonal(form, n):
    RUN[form](n)


@pytest.mark.parametrize("form", ["rv_b64", "mask_b64", "mask_json"])
def test_accepted_on_a_small_prime(form):
    """The ACCEPTED cases on a !BIG prime (a refusal does not depend on the field; what an
    accepted text decodes to reaches the field arithmetic): verdicts and outputs vs Python ints."""
    small = TC.PRIMES[1]
    assert not FC.BY_ID[small].big and FC.BY_ID[PID].big
    for n in TC.PARTIES:
        run_single_wire(form, n, small, "accepted")
