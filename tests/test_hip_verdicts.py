"""The verdict matrix: every verifying call of the C ABI (every declaration
with a `first_fail`: the table MATRIX of tests/verdict_cases.py, held against
the headers by tests/test_session_cases_cpu.py), in every party-count
form (templated 1-4, the run-time loop at 5 and 16) and both prime classes
(`test` is BIG, `m89` is !BIG and has room for + k p), on the catalogue of
tests/verdict_cases.py -- a fault in each of the five MAC fields is rejected at
its word, every change that is no fault mod p is accepted, crossed and
compensated MACs get the verdict of the words that were read, and of several
faults in different fields the smallest index wins.

Every expected verdict and every expected output word comes from ``%`` on
Python ints through tests/verdict_cases.py (tests/test_verdict_cpu.py pins
the catalogue itself); wire texts are Python's base64 of the edited arrays.
No result is compared with another call of the library.  The outputs are
compared whole for rejected inputs too: the headers promise that they are
written whatever the verdict.  The client session is the exception the header
states: its host-mode finish calls write no output on a rejection (checked on
pre-filled buffers), its device-mode ones write everything; its parties arrive
in an order that rotates with the case, and for every rejected case
amph_client_word at the failing word gives the five recombined values of the
edited rows -- the numbers the reference's failure message is rendered from,
which crossed and compensated MACs tell apart from a read of the wrong column.

Single-object calls run 1,217 words (a 1,024-lane workgroup edge, six 192-word
wire tiles and a 65-word tail, base64 padding present); the packed and batch
calls hold the whole catalogue in one launch, one 257-word object per case, so
objects are not aligned with waves.

The K-secret client session (amph_clients_*) takes the catalogue as the objects
of ONE session (tests/verdict_cases.py session_objects): the 257-word objects
with an honest filler of 0 to 385 words after each, so that the per-object
192-word tiles of its accumulate and mask kernels have uneven prefix sums, empty
objects stand next to failing ones and no failing object starts at word 0.  Its
first_fails are object-local; it writes every object's outputs in both modes,
and they are compared whole.
"""
import base64
import ctypes as C
import functools
import json
import os
import uuid

import numpy as np
import pytest

from oracle import amphora_oracle as O
from tests import field_cases as FC
from tests import verdict_cases as VC
from tests.test_hip_primes import NF, verdict

pytestmark = pytest.mark.gpu

PRIMES = ["test", "m89"]
W_SINGLE, W_OBJECT = 1217, 257
N_SECRETS_SHORT = 700  # mask_input with a verify-only tail of 517 words
SMALL_SIZES = [1, 192]  # one word; one whole wire tile (no base64 padding)
BATCH_WORDS = 256  # the host pipeline's batch in these tests
DEFAULT_BATCH_WORDS = 4 << 20  # capi_internal.hpp
SINGLE_CALLS = ["recombine_verify", "mask_input", "verify", "recombine_verify_b64", "mask_input_b64", "mask_input_json",
                "client_verify", "client_mask", "client_mask_json"]
MANY_CALLS = ["packed", "batch", "wire_packed", "wire_batch", "upload_packed", "upload_batch",
              "clients_verify", "clients_mask", "clients_mask_json"]
OK, E_VERIFY = 0, 1


# ---- contexts -------------------------------------------------------------------------
_CTX = {}


def _ctx(pid, kind="plain"):
    """plain; pipeline: no small-call arena, so host calls take the batched
    pipeline; multi: two shards on one GPU.  Made once per module and released
    with it (`_release`)."""
    if (pid, kind) not in _CTX:
        import torch
        assert torch.cuda.is_available()
        import amphora_amd
        pr = FC.BY_ID[pid]
        old = os.environ.get("AMPH_SMALL_BYTES")
        if kind == "pipeline":
            os.environ["AMPH_SMALL_BYTES"] = "0"  # read when the context is created
        try:
            _CTX[pid, kind] = amphora_amd.Context(pr.p, pr.r, pr.rinv, devices=[0, 0] if kind == "multi" else None)
        finally:
            if kind == "pipeline":
                if old is None:
                    del os.environ["AMPH_SMALL_BYTES"]
                else:
                    os.environ["AMPH_SMALL_BYTES"] = old
    return _CTX[pid, kind]


@pytest.fixture(scope="module", autouse=True)
def _release():
    """The contexts (their streams and workers) and the cached device copies
    end with this module: later modules start from the process as it was."""
    yield
    import gc
    _CTX.clear()
    rows.cache_clear()
    many.cache_clear()
    clients.cache_clear()
    gc.collect()


def up(a):
    """A fresh device copy (the catalogue's arrays are read-only)."""
    import torch
    a = np.array(a, copy=True)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


def down(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def verdicts(ff):
    """A verdict array of either mode as a list of -1 / index."""
    if not isinstance(ff, np.ndarray):
        ff = down(ff)
    return [-1 if int(v) == NF else int(v) for v in ff]


def record_rows(words16):
    """Python's base64 of each 16-byte word: the (W, 24) records."""
    raw = b"".join(base64.b64encode(bytes(w)) for w in np.asarray(words16))
    return np.frombuffer(raw, np.uint8).reshape(-1, 24).copy()


def data_text(records) -> bytes:
    """Jackson's compact MaskedInput "data" array of the given records."""
    return b"[" + b",".join(b'{"value":"' + bytes(r) + b'"}' for r in np.asarray(records)) + b"]"


def decoded_records(text: bytes):
    """The "data" array text parsed with Python: the 16-byte words it carries."""
    return [int.from_bytes(base64.b64decode(e["value"], validate=True), "little") for e in json.loads(text)]


# ---- one (prime, n, W): the base in every representation, built once ----------------------
class Rows:
    def __init__(self, pid, n, W, classes="ABCDE"):
        self.pr = FC.BY_ID[pid]
        self.b, self.cases = VC.catalogue(pid, n, W, classes)
        self.W, self.n = W, n
        self.arrays = VC.base_arrays(self.b)
        self.secrets = VC.secrets_for(self.b)
        self.sec = FC.arr(self.secrets)
        self.y = FC.arr(self.b.cols[VC.Y])
        self.m = FC.arr(FC.mask_words(self.pr, self.secrets, self.b.cols[VC.Y]))
        self.rec = record_rows(self.m)
        self.texts = [[VC.b64(f) for f in o] for o in self.arrays]
        self.col_arrays = [FC.arr(col) for col in self.b.cols]
        for a in (self.sec, self.y, self.m, self.rec, *self.col_arrays):
            a.setflags(write=False)
        self._dev = self._dev_texts = self._dev_sec = None

    # expected outputs of a case: the base's with the changed secrets patched in
    def want_y(self, e):
        out = self.y.copy()
        for i, y in e.changed.items():
            out[i] = FC.arr([y])[0]
        return out

    def want_m(self, e):
        out = self.m.copy()
        for i, y in e.changed.items():
            out[i] = FC.arr(FC.mask_words(self.pr, [self.secrets[i]], [y]))[0]
        return out

    def want_rec(self, e):
        out = self.rec.copy()
        for i in e.changed:
            out[i] = record_rows(self.want_m(e)[i:i + 1])[0]
        return out

    # inputs of a case in each representation: only the edited fields are rebuilt
    def host(self, case):
        return VC.apply(self.arrays, case)[0]

    def device(self, case):
        if self._dev is None:
            self._dev = [[up(f) for f in o] for o in self.arrays]
        arrays, hit = VC.apply(self.arrays, case)
        out = [list(o) for o in self._dev]
        for j, k in hit:
            out[j][k] = up(arrays[j][k])
        return out

    def host_texts(self, case):
        arrays, hit = VC.apply(self.arrays, case)
        out = [list(o) for o in self.texts]
        for j, k in hit:
            out[j][k] = VC.b64(arrays[j][k])
        return out

    def device_texts(self, case):
        as_dev = lambda t: up(np.frombuffer(t, np.uint8))  # noqa: E731
        if self._dev_texts is None:
            self._dev_texts = [[as_dev(t) for t in o] for o in self.texts]
        arrays, hit = VC.apply(self.arrays, case)
        out = [list(o) for o in self._dev_texts]
        for j, k in hit:
            out[j][k] = as_dev(VC.b64(arrays[j][k]))
        return out

    def dev_sec(self):
        if self._dev_sec is None:
            self._dev_sec = up(self.sec)
        return self._dev_sec

    def columns(self, case):
        """[y, r, v, w, u] canonical (W, 16) arrays of the edited rows."""
        cols = VC.columns(self.b, case)
        out = []
        for k in range(5):
            a = self.col_arrays[k]
            idx = [i for i in {e[2] for e in case.edits} if cols[k][i] != self.b.cols[k][i]]
            if idx:
                a = a.copy()
                for i in idx:
                    a[i] = FC.arr([cols[k][i]])[0]
            out.append(a)
        return out


@functools.lru_cache(maxsize=None)
def rows(pid, n, W=W_SINGLE, classes="ABCDE"):
    return Rows(pid, n, W, classes)


# ---- single-object calls ----------------------------------------------------------------
def word_modes(pid):
    """(mode, context, places the inputs): the host small call, the host
    pipeline in 256-word batches, the device call."""
    return [("host", _ctx(pid), False), ("pipeline", _ctx(pid, "pipeline"), False), ("device", _ctx(pid), True)]


def run_recombine_verify(pid, n):
    R = rows(pid, n)
    names = [c.name for c, _ in R.cases]
    # an order case whose faults lie in different pipeline batches
    assert "E_1023v_1024u" in names and 1023 // BATCH_WORDS != 1024 // BATCH_WORDS
    pipe = _ctx(pid, "pipeline")
    pipe.set_batch_words(BATCH_WORDS)
    try:
        for mode, ctx, on_dev in word_modes(pid):
            for c, e in R.cases:
                y, ff = ctx.recombine_verify(R.device(c) if on_dev else R.host(c))
                assert verdict(ff) == e.ff, (mode, c.name, verdict(ff), e.ff)
                assert np.array_equal(down(y) if on_dev else y, R.want_y(e)), (mode, c.name)
    finally:
        pipe.set_batch_words(DEFAULT_BATCH_WORDS)


def run_mask_input(pid, n):
    R = rows(pid, n)
    S = N_SECRETS_SHORT
    # the verify-only tail's first word and the last lane of its first wave, in the fields the
    # tail alone still reads for the verdict
    tail = [VC.single_fault(R.b, k, i, party=(i + k) % n, name="tail_%s_%d" % (VC.FIELDS[k], i))
            for k in (VC.U, VC.V, VC.R) for i in (S, S + 63)]
    tail = [(c, VC.expect(R.b, c)) for c in tail]
    assert [e.ff for _, e in tail] == [S, S + 63] * 3 and S + 63 < R.W
    pipe = _ctx(pid, "pipeline")
    pipe.set_batch_words(BATCH_WORDS)
    try:
        for mode, ctx, on_dev in word_modes(pid):
            sec = R.dev_sec() if on_dev else R.sec
            for c, e in R.cases:
                m, ff = ctx.mask_input(R.device(c) if on_dev else R.host(c), sec)
                assert verdict(ff) == e.ff, (mode, c.name, verdict(ff), e.ff)
                assert np.array_equal(down(m) if on_dev else m, R.want_m(e)), (mode, c.name)
            short = [(c, e) for c, e in R.cases if c.cls in "AD"] + tail
            for c, e in short:
                m, ff = ctx.mask_input(R.device(c) if on_dev else R.host(c), sec[:S])
                assert verdict(ff) == e.ff, (mode, "short", c.name, verdict(ff), e.ff)
                assert np.array_equal(down(m) if on_dev else m, R.want_m(e)[:S]), (mode, "short", c.name)
    finally:
        pipe.set_batch_words(DEFAULT_BATCH_WORDS)


def run_verify(pid, n):
    """amph_verify over the recombined columns, in the Java method's argument
    order (secrets, rs, us, vs, ws); class B changes no recombined value."""
    R = rows(pid, n)
    ctx = _ctx(pid)
    picked = [(c, e) for c, e in R.cases if c.cls in "ACDE"]
    assert {VC.FIELDS[c.edits[0][1]] for c, _ in picked if c.cls == "A"} == set(VC.FIELDS)
    for c, e in picked:
        y, r, v, w, u = R.columns(c)
        assert ctx.verify(y, r, u, v, w) == e.ff, ("host", c.name)
        assert verdict(ctx.verify(*[up(x) for x in (y, r, u, v, w)])) == e.ff, ("device", c.name)


def wire_sizes(pid, n):
    """The full catalogue at 1,217 words, the A cases at 1 and at 192 words."""
    return [rows(pid, n)] + [rows(pid, n, W, "A") for W in SMALL_SIZES]


def run_recombine_verify_b64(pid, n):
    ctx = _ctx(pid)
    for R in wire_sizes(pid, n):
        for on_dev in (False, True):
            for c, e in R.cases:
                y, ff, bad = ctx.recombine_verify_b64(R.device_texts(c) if on_dev else R.host_texts(c), R.W)
                assert verdict(ff) == e.ff and verdict(bad) == -1, (R.W, on_dev, c.name, verdict(ff), e.ff)
                assert np.array_equal(down(y) if on_dev else y, R.want_y(e)), (R.W, on_dev, c.name)


def run_mask_input_b64(pid, n):
    ctx = _ctx(pid)
    for R in wire_sizes(pid, n):
        for on_dev in (False, True):
            sec = R.dev_sec() if on_dev else R.sec
            get = down if on_dev else (lambda a: a)
            for c, e in R.cases:
                tx = R.device_texts(c) if on_dev else R.host_texts(c)
                m16, rec, ff, bad = ctx.mask_input_b64(tx, R.W, sec, records=True, raw=True)
                assert verdict(ff) == e.ff and verdict(bad) == -1, (R.W, on_dev, c.name, verdict(ff), e.ff)
                assert np.array_equal(get(m16), R.want_m(e)), (R.W, on_dev, c.name)
                assert np.array_equal(get(rec), R.want_rec(e)), (R.W, on_dev, c.name)
                _, rec, ff, bad = ctx.mask_input_b64(tx, R.W, sec)  # records only: the client's form
                assert verdict(ff) == e.ff and verdict(bad) == -1, (R.W, on_dev, c.name)
                assert np.array_equal(get(rec), R.want_rec(e)), (R.W, on_dev, c.name)


def run_mask_input_json(pid, n):
    ctx = _ctx(pid)
    for R in wire_sizes(pid, n):
        assert decoded_records(data_text(R.rec)) == FC.mask_words(R.pr, R.secrets, R.b.cols[VC.Y])
        for on_dev in (False, True):
            sec = R.dev_sec() if on_dev else R.sec
            for c, e in R.cases:
                text, ff, bad = ctx.mask_input_json(R.device_texts(c) if on_dev else R.host_texts(c), R.W, sec)
                assert verdict(ff) == e.ff and verdict(bad) == -1, (R.W, on_dev, c.name, verdict(ff), e.ff)
                text = down(text).tobytes() if on_dev else text
                assert text == data_text(R.want_rec(e)), (R.W, on_dev, c.name)


# ---- the client session: the same texts, one party at a time ------------------------------------
def arrival_order(n, q, case):
    """Rotates with the case index: forward, reverse, the edited party first."""
    fwd = list(range(n))
    if q % 3 == 0:
        return fwd
    if q % 3 == 1:
        return fwd[::-1]
    first = case.edits[0][0]
    return [first] + [j for j in fwd if j != first]


def run_client(pid, n, finish):
    """amph_client_finish_verify / _mask / _mask_json (`finish`) and their _dev
    forms over sums accumulated in a rotating arrival order.  Device mode: the
    outputs whole, for rejected cases too.  Host mode, through the C ABI with
    pre-filled buffers: a rejected case leaves them as they were.  Every
    rejected case: amph_client_word at the failing word gives the five
    recombined values of the edited rows -- what the failure message shows;
    for classes C and D at every edited word."""
    import amphora_amd
    lib = amphora_amd._lib.lib
    R = rows(pid, n)
    ctx = _ctx(pid)
    W = R.W
    orders = set()
    for on_dev in (False, True):
        for q, (c, e) in enumerate(R.cases):
            order = arrival_order(n, q, c)
            orders.add(tuple(order))
            texts = R.device_texts(c) if on_dev else R.host_texts(c)
            tag = ("device" if on_dev else "host", c.name, order)
            s = ctx.client_begin_dev(W, n) if on_dev else ctx.client_begin(W, n)
            try:
                bads = [s.party(j, texts[j]) for j in order]
                if on_dev:
                    if finish == "verify":
                        y, ff, bad = s.finish_verify()
                        got, want = [down(y)], [R.want_y(e)]
                    elif finish == "mask":
                        m16, rec, ff, bad = s.finish_mask(R.dev_sec(), records=True, raw=True)
                        got, want = [down(m16), down(rec)], [R.want_m(e), R.want_rec(e)]
                    else:
                        text, ff, bad = s.finish_mask_json(R.dev_sec())
                        got, want = [down(text).tobytes()], [data_text(R.want_rec(e))]
                    assert verdict(ff) == e.ff and verdict(bad) == -1, (tag, verdict(ff), e.ff)
                    assert all(verdict(b) == -1 for b in bads), tag
                    for g, w in zip(got, want):  # written whatever the verdict
                        assert np.array_equal(g, w) if isinstance(w, np.ndarray) else g == w, tag
                else:
                    assert bads == [-1] * n, tag
                    ff, bad = C.c_int64(-7), C.c_int64(-7)
                    if finish == "verify":
                        outs, want = [np.full((W, 16), 0xA5, np.uint8)], [R.want_y(e)]
                        st = lib.amph_client_finish_verify(s._h, outs[0].ctypes.data, C.byref(ff), C.byref(bad))
                    elif finish == "mask":
                        outs = [np.full((W, 16), 0xA5, np.uint8), np.full((W, 24), 0xA5, np.uint8)]
                        want = [R.want_m(e), R.want_rec(e)]
                        st = lib.amph_client_finish_mask(s._h, R.sec.ctypes.data, W, outs[0].ctypes.data,
                                                         outs[1].ctypes.data, C.byref(ff), C.byref(bad))
                    else:
                        cap = 37 * W + 1
                        outs = [np.full(cap, 0xA5, np.uint8)]
                        want = [np.frombuffer(data_text(R.want_rec(e)), np.uint8)]
                        st = lib.amph_client_finish_mask_json(s._h, R.sec.ctypes.data, W, outs[0].ctypes.data, cap,
                                                              C.byref(ff), C.byref(bad))
                    assert (st, ff.value, bad.value) == (E_VERIFY if e.ff >= 0 else OK, e.ff, -1), (tag, st, ff.value)
                    for g, w in zip(outs, want):
                        if e.ff >= 0:
                            assert (g == 0xA5).all(), tag  # host mode writes no output on an error
                        else:
                            assert g.shape == w.shape and np.array_equal(g, w), tag
                at = ({e.ff} if e.ff >= 0 else set()) | ({ed[2] for ed in c.edits} if c.cls in "CD" else set())
                if at:  # (the compensated MACs of class D are accepted: their edited words are read back as well)
                    cols = VC.columns(R.b, c)
                    for i in sorted(at):
                        assert s.word(i) == tuple(cols[k][i] for k in range(5)), (tag, i)
            finally:
                s.close()
    if n >= 3:
        assert len(orders) >= 3  # forward, reverse and at least one "edited party first" that is neither


# ---- many objects per launch: one object per case -------------------------------------------
class Many:
    """The catalogue at 257 words as objects of one launch: an honest object,
    one object per case, and a pair -- `u` off in the last word of one object,
    `w` off in the first word of the next -- whose two words share a wave.
    `gaps` puts two empty objects after every object."""

    def __init__(self, pid, n, gaps, shift=0):
        R = self.R = rows(pid, n, W_OBJECT)
        W = R.W
        honest = VC.Case("honest", "B", (), -1, frozenset(), None)
        pair = [VC.single_fault(R.b, VC.U, W - 1, party=n - 1, name="pair_last_u"),
                VC.single_fault(R.b, VC.Wf, 0, party=0, name="pair_first_w")]
        listed = [(honest, VC.Expect(-1, {}))] + list(R.cases) + [(c, VC.expect(R.b, c)) for c in pair]
        listed = listed[shift:] + listed[:shift]  # another assignment of cases to objects (the accumulate pass)
        self.names, self.sizes, self.ff = [], [], []
        self.objects, self.secrets, self.y, self.m, self.rec, self.texts = [], [], [], [], [], []
        e16 = np.zeros((0, 16), np.uint8)
        for c, e in listed:
            self.names.append(c.name)
            self.sizes.append(W)
            self.ff.append(e.ff)
            self.objects.append(R.host(c) if c.edits else [list(o) for o in R.arrays])
            self.texts.append(R.host_texts(c) if c.edits else R.texts)
            self.secrets.append(R.sec)
            self.y.append(R.want_y(e))
            self.m.append(R.want_m(e))
            self.rec.append(R.want_rec(e))
            for _ in range(2 if gaps else 0):
                self.names.append("empty")
                self.sizes.append(0)
                self.ff.append(-1)
                self.objects.append([[e16] * 5 for _ in range(n)])
                self.texts.append([[b""] * 5 for _ in range(n)])
                self.secrets.append(e16)
                self.y.append(e16)
                self.m.append(e16)
                self.rec.append(np.zeros((0, 24), np.uint8))
        self.K = len(self.sizes)
        self.woff = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.uint64)
        if shift == 0:  # on the inputs: the pair's two words are neighbours inside one wave
            lo, hi = self.names.index("pair_last_u"), self.names.index("pair_first_w")
            g = int(self.woff[lo + 1]) - 1
            assert int(self.woff[hi]) == g + 1 and g // 64 == (g + 1) // 64 and self.ff[lo] == W - 1 and self.ff[hi] == 0
        self.packed = [[np.ascontiguousarray(np.concatenate([obj[j][k] for obj in self.objects])) for k in range(5)]
                       for j in range(n)]
        self.packed_sec = np.ascontiguousarray(np.concatenate(self.secrets))
        self.packed_y = np.concatenate(self.y)
        self.packed_m = np.concatenate(self.m)
        self.packed_rec = np.concatenate(self.rec)

    def split(self, a):
        return [np.asarray(a)[int(self.woff[o]):int(self.woff[o + 1])] for o in range(self.K)]


@functools.lru_cache(maxsize=None)
def many(pid, n, gaps, shift=0):
    return Many(pid, n, gaps, shift)


def run_packed(pid, n):
    import torch
    ctx = _ctx(pid)
    M = many(pid, n, True)
    y, ff = ctx.recombine_verify_packed(M.packed, M.woff)
    assert verdicts(ff) == M.ff and np.array_equal(y, M.packed_y), "host"
    m, ff = ctx.mask_input_packed(M.packed, M.woff, M.packed_sec)
    assert verdicts(ff) == M.ff and np.array_equal(m, M.packed_m), "host"
    d = [[up(f) for f in o] for o in M.packed]
    off, sec = up(M.woff), up(M.packed_sec)
    y, ff = ctx.recombine_verify_packed(d, off)
    assert verdicts(ff) == M.ff and np.array_equal(down(y), M.packed_y), "device"
    m, ff = ctx.mask_input_packed(d, off, sec)
    assert verdicts(ff) == M.ff and np.array_equal(down(m), M.packed_m), "device"
    # AMPH_F_ACCUMULATE over two passes: the element-wise minimum of two REFERENCE verdict lists
    M2 = many(pid, n, True, shift=7)
    assert M2.sizes == M.sizes and M2.ff != M.ff
    want = [min([x for x in pair if x >= 0], default=-1) for pair in zip(M.ff, M2.ff)]
    assert want != M.ff and want != M2.ff  # both passes show
    d2 = [[up(f) for f in o] for o in M2.packed]
    for masked in (False, True):
        acc = torch.full((M.K,), NF, dtype=torch.int64, device="cuda")
        for dd, MM in ((d, M), (d2, M2)):
            if masked:
                out, _ = ctx.mask_input_packed(dd, off, sec, first_fail=acc, accumulate=True)
            else:
                out, _ = ctx.recombine_verify_packed(dd, off, first_fail=acc, accumulate=True)
            assert np.array_equal(down(out), MM.packed_m if masked else MM.packed_y), masked
        assert verdicts(acc) == want, masked


def run_batch(pid, n):
    ctx = _ctx(pid)
    M = many(pid, n, True)
    ys, ff = ctx.recombine_verify_batch(M.objects)
    assert verdicts(ff) == M.ff
    assert all(g.shape == w.shape and np.array_equal(g, w) for g, w in zip(ys, M.y))
    ms, ff = ctx.mask_input_batch(M.objects, M.secrets)
    assert verdicts(ff) == M.ff
    assert all(g.shape == w.shape and np.array_equal(g, w) for g, w in zip(ms, M.m))


def wire_buffers(M, slot_chars):
    """(text offsets, per party the five field buffers): object o's text at the
    sum of its predecessors' amph_wire_slot_chars, '!' between the texts."""
    toff = np.concatenate([[0], np.cumsum([slot_chars(W) for W in M.sizes])]).astype(np.uint64)[:M.K]
    nchars = int(toff[-1]) + len(M.texts[-1][0][0])
    bufs = []
    for j in range(M.R.n):
        fs = []
        for k in range(5):
            buf = np.full(nchars, ord("!"), np.uint8)
            for o in range(M.K):
                t = M.texts[o][j][k]
                buf[int(toff[o]):int(toff[o]) + len(t)] = np.frombuffer(t, np.uint8)
            fs.append(buf)
        bufs.append(fs)
    return toff, bufs


def run_wire_packed(pid, n):
    import amphora_amd
    ctx = _ctx(pid)
    M = many(pid, n, False)
    toff, bufs = wire_buffers(M, amphora_amd._lib.wire_slot_chars)
    assert all(int(t) % 16 == 0 for t in toff)
    clean = [-1] * M.K
    for on_dev in (False, True):
        get = down if on_dev else (lambda a: a)
        tx = [[up(f) for f in o] for o in bufs] if on_dev else bufs
        wo, to = (up(M.woff), up(toff)) if on_dev else (M.woff, toff)
        sec = up(M.packed_sec) if on_dev else M.packed_sec
        y, ff, bad = ctx.recombine_verify_b64_packed(tx, wo, to)
        assert verdicts(ff) == M.ff and verdicts(bad) == clean, on_dev
        assert np.array_equal(get(y), M.packed_y), on_dev
        m16, rec, ff, bad = ctx.mask_input_b64_packed(tx, wo, to, sec, records=True, raw=True)
        assert verdicts(ff) == M.ff and verdicts(bad) == clean, on_dev
        assert np.array_equal(get(m16), M.packed_m) and np.array_equal(get(rec), M.packed_rec), on_dev
        text, oo, ff, bad = ctx.mask_input_json_packed(tx, wo, to, sec)
        assert verdicts(ff) == M.ff and verdicts(bad) == clean, on_dev
        text, oo = get(text), get(oo)
        for o in range(M.K):
            want = data_text(M.rec[o])
            assert text[int(oo[o]):int(oo[o]) + len(want)].tobytes() == want, (on_dev, M.names[o])


def run_wire_batch(pid, n):
    ctx = _ctx(pid)
    M = many(pid, n, False)
    clean = [-1] * M.K
    ys, ff, bad = ctx.recombine_verify_b64_batch(M.texts, M.sizes)
    assert verdicts(ff) == M.ff and verdicts(bad) == clean
    assert all(np.array_equal(g, w) for g, w in zip(ys, M.y))
    m16, rec, ff, bad = ctx.mask_input_b64_batch(M.texts, M.sizes, M.secrets, records=True, raw=True)
    assert verdicts(ff) == M.ff and verdicts(bad) == clean
    assert all(np.array_equal(g, w) for g, w in zip(m16, M.m)) and all(np.array_equal(g, w) for g, w in zip(rec, M.rec))
    texts, ff, bad = ctx.mask_input_json_batch(M.texts, M.sizes, M.secrets)
    assert verdicts(ff) == M.ff and verdicts(bad) == clean
    assert texts == [data_text(r) for r in M.rec]


def upload_texts(M):
    """Each object's expected "data" array text, from Python ints: the masked
    words of the catalogue (FC.mask_words), Python's base64 and the frame."""
    out = []
    for o in range(M.K):
        words = FC.ints(M.m[o])
        text = data_text(record_rows(FC.arr(words)))
        assert decoded_records(text) == words and len(text) == 37 * len(words) + 1
        out.append(text)
    return out


def run_upload_packed(pid, n):
    """amph_mask_input_json_packed: one 257-word object per case."""
    import amphora_amd
    ctx = _ctx(pid)
    M = many(pid, n, False)
    want = upload_texts(M)
    toff, bufs = wire_buffers(M, amphora_amd._lib.wire_slot_chars)
    clean = [-1] * M.K
    for on_dev in (False, True):
        get = down if on_dev else (lambda a: a)
        tx = [[up(f) for f in o] for o in bufs] if on_dev else bufs
        wo, to = (up(M.woff), up(toff)) if on_dev else (M.woff, toff)
        sec = up(M.packed_sec) if on_dev else M.packed_sec
        text, oo, ff, bad = ctx.mask_input_json_packed(tx, wo, to, sec)
        assert verdicts(ff) == M.ff and verdicts(bad) == clean, on_dev
        text, oo = get(text), [int(x) for x in get(oo)]
        assert oo == [o * amphora_amd._lib.upload_slot_chars(W_OBJECT) for o in range(M.K)], on_dev
        for o in range(M.K):  # written whatever the object's verdict
            assert text[oo[o]:oo[o] + len(want[o])].tobytes() == want[o], (on_dev, M.names[o])
    # AMPH_F_ACCUMULATE over two passes: the element-wise minimum of two REFERENCE verdict lists
    import torch
    M2 = many(pid, n, False, shift=7)
    both = [min([x for x in pair if x >= 0], default=-1) for pair in zip(M.ff, M2.ff)]
    assert M2.sizes == M.sizes and both != M.ff and both != M2.ff
    acc = torch.full((M.K,), NF, dtype=torch.int64, device="cuda")
    seen = torch.full((M.K,), NF, dtype=torch.int64, device="cuda")
    for MM in (M, M2):
        t2, b2 = wire_buffers(MM, amphora_amd._lib.wire_slot_chars)
        text, oo, _, _ = ctx.mask_input_json_packed([[up(f) for f in o] for o in b2], up(MM.woff), up(t2),
                                                    up(MM.packed_sec), first_fail=acc, bad_char=seen, accumulate=True)
        text, oo = down(text), [int(x) for x in down(oo)]
        for o, w in enumerate(upload_texts(MM)):
            assert text[oo[o]:oo[o] + len(w)].tobytes() == w, (MM.names[o], "accumulate")
    assert verdicts(acc) == both and verdicts(seen) == clean


def run_upload_batch(pid, n):
    """amph_mask_input_json_batch: the same objects, gathered from their own host buffers."""
    ctx = _ctx(pid)
    M = many(pid, n, False)
    texts, ff, bad = ctx.mask_input_json_batch(M.texts, M.sizes, M.secrets)
    assert verdicts(ff) == M.ff and verdicts(bad) == [-1] * M.K
    assert texts == upload_texts(M)


# ---- the K-secret client session: the catalogue as the objects of ONE session -------------------------
PREFILL = 0xA5
CLIENTS_MESSAGE = "Verification of secret has failed: object %d at word %d (%d of %d objects failed)"


class Clients:
    """VC.session_objects(pid, n) in the arrays a session takes and gives: per
    party the five slotted buffers in the dense layout ('!' in every gap and in
    the tail), the packed secrets, and every expected output whole -- all from
    the builder's Python-int references."""

    def __init__(self, pid, n):
        S = self.S = VC.session_objects(pid, n)
        self.K, self.T = len(S.sizes), S.woff[-1]
        self.woff = np.asarray(S.woff, np.uint64)
        self.foff = np.asarray(S.foff, np.uint64)
        self.bufs = [[np.full(S.field_chars, ord("!"), np.uint8) for _ in range(5)] for _ in range(n)]
        for o, obj in enumerate(S.objects):
            at, nc = S.foff[o], VC.wire_text_chars(S.sizes[o])
            for j, five in enumerate(VC.object_texts(obj)):
                for k, t in enumerate(five):
                    assert len(t) == nc
                    self.bufs[j][k][at:at + nc] = np.frombuffer(t, np.uint8)
        def packed(words_of):
            made = {}  # (most objects share their base's words: each distinct tuple becomes an array once)
            for t in map(words_of, S.objects):
                if t not in made:
                    made[t] = FC.arr(t)
            return np.concatenate([made[words_of(obj)] for obj in S.objects])

        self.sec = packed(lambda obj: obj.secrets)
        self.y = packed(lambda obj: obj.y)
        self.m = packed(lambda obj: obj.masked)
        assert self.sec.shape == self.y.shape == self.m.shape == (self.T, 16)
        self.rec = np.frombuffer(b"".join(obj.records for obj in S.objects), np.uint8).reshape(self.T, 24)
        # the framed texts in the dense upload layout; what lies between them stays as pre-filled
        self.text = np.full(S.upload_chars, PREFILL, np.uint8)
        for o, obj in enumerate(S.objects):
            assert len(obj.text) == VC.upload_text_chars(S.sizes[o]) and (S.sizes[o] > 0 or obj.text == b"[]")
            self.text[S.uoff[o]:S.uoff[o] + len(obj.text)] = np.frombuffer(obj.text, np.uint8)
        failing = [o for o in range(self.K) if S.ff[o] >= 0]
        self.status = (E_VERIFY, CLIENTS_MESSAGE % (failing[0], S.ff[failing[0]], len(failing), self.K))
        # the words read back: every rejected object's failing word, every edited word of classes C and D
        self.reads = []
        for o, obj in enumerate(S.objects):
            at = ({obj.ff} if obj.ff >= 0 else set()) | \
                ({e[2] for e in obj.case.edits} if obj.kind == "case" and obj.case.cls in "CD" else set())
            self.reads += [(o, i, tuple(obj.cols[k][i] for k in range(5))) for i in sorted(at)]
        assert {S.objects[o].case.cls for o, _, _ in self.reads} == set("ACDE") and len(self.reads) > len(failing)
        self._dev = None

    def device(self):
        """(the parties' buffers, the secrets) on the device, uploaded once."""
        if self._dev is None:
            self._dev = ([[up(f) for f in five] for five in self.bufs], up(self.sec))
        return self._dev


@functools.lru_cache(maxsize=2)  # (the three finishes of one prime and party count run in a row)
def clients(pid, n):
    return Clients(pid, n)


def run_clients(pid, n, finish):
    """amph_clients_finish_verify / _mask / _mask_json (`finish`) and their _dev
    forms on the objects of VC.session_objects: host mode in every order of
    FC.session_orders(n), device mode in the last one (at most four sessions).
    Per object: the verdict is the builder's, no illegal character is reported
    by any call, and the outputs are the builder's WHOLE -- the K session writes
    every object's outputs whatever its verdict, in both modes, "[]" for an
    empty object, nothing between the framed texts.  Host status and message
    follow from the reference verdict list; amph_clients_word gives the five
    recombined values of the edited rows.  Last, and weaker: the verdict arrays
    are those of the packed wire-text call on the same buffers."""
    M = clients(pid, n)
    S = M.S
    ctx = _ctx(pid)
    clean = [-1] * M.K
    orders = FC.session_orders(n)
    runs = [(False, order) for order in orders] + [(True, orders[-1])]
    assert len(runs) <= 4 and sum(f >= 0 for f in S.ff) >= 20
    host_verdicts = None
    for on_dev, order in runs:
        tag = ("device" if on_dev else "host", order)
        bufs, sec = M.device() if on_dev else (M.bufs, M.sec)
        with (ctx.clients_begin_dev(M.woff, n) if on_dev else ctx.clients_begin(M.woff, n)) as s:
            # the dense layout, computed in Python from the word counts alone
            assert (s.field_chars, s.upload_chars) == (S.field_chars, S.upload_chars), tag
            assert s.field_offsets.tolist() == list(S.foff) and s.upload_offsets.tolist() == list(S.uoff), tag
            parts = [s.party(j, bufs[j]) if on_dev else s.party(j, bufs[j], status=True) for j in order]
            if finish == "verify":
                res, want = s.finish_verify(status=True), [M.y]
            elif finish == "mask":
                res, want = s.finish_mask(sec, records=True, raw=True, status=True), [M.m, M.rec]
            else:
                out = np.full(S.upload_chars, PREFILL, np.uint8)
                res, want = s.finish_mask_json(sec, out=up(out) if on_dev else out, status=True), [M.text]
            *outs, ff, bad, status = res
            if on_dev:
                assert status[0] == OK and all(verdicts(v) == clean for v in parts), tag
                outs = [down(x) for x in outs]
            else:
                assert all(v.tolist() == clean and st == (OK, "") for v, st in parts), tag
                assert status == M.status, (tag, status)
                host_verdicts = (ff, bad)
            assert verdicts(ff) == list(S.ff), (tag, verdicts(ff))
            assert verdicts(bad) == clean, tag
            for g, w in zip(outs, want):  # whole: rejected objects, empty objects and the gaps included
                if not (g.shape == w.shape and np.array_equal(g, w)):
                    where = np.flatnonzero((g != w).reshape(len(w), -1).any(axis=1))
                    raise AssertionError((tag, "first difference at row %d of %d" % (where[0], len(w))))
            for o, i, cols in M.reads:
                assert s.word(o, i) == cols, (tag, S.objects[o].name, i)
    # bit for bit what the packed wire-text call says on all parties' buffers at once
    if finish == "verify":
        _, ff, bad = ctx.recombine_verify_b64_packed(M.bufs, M.woff, M.foff)
    elif finish == "mask":
        _, _, ff, bad = ctx.mask_input_b64_packed(M.bufs, M.woff, M.foff, M.sec, records=True, raw=True)
    else:
        _, _, ff, bad = ctx.mask_input_json_packed(M.bufs, M.woff, M.foff, M.sec)
    assert np.array_equal(host_verdicts[0], ff) and np.array_equal(host_verdicts[1], bad)


RUN = {"recombine_verify": run_recombine_verify, "mask_input": run_mask_input, "verify": run_verify,
       "recombine_verify_b64": run_recombine_verify_b64, "mask_input_b64": run_mask_input_b64,
       "mask_input_json": run_mask_input_json, "packed": run_packed, "batch": run_batch,
       "wire_packed": run_wire_packed, "wire_batch": run_wire_batch,
       "client_verify": functools.partial(run_client, finish="verify"),
       "client_mask": functools.partial(run_client, finish="mask"),
       "client_mask_json": functools.partial(run_client, finish="mask_json"),
       "upload_packed": run_upload_packed, "upload_batch": run_upload_batch,
       "clients_verify": functools.partial(run_clients, finish="verify"),
       "clients_mask": functools.partial(run_clients, finish="mask"),
       "clients_mask_json": functools.partial(run_clients, finish="mask_json")}
assert list(RUN) and set(RUN) == set(VC.MATRIX.values()) == set(SINGLE_CALLS + MANY_CALLS)


@pytest.mark.parametrize("call", SINGLE_CALLS + MANY_CALLS)
@pytest.mark.parametrize("n", FC.PARTY_COUNTS)
@pytest.mark.parametrize("pid", PRIMES)
def test_verdicts(pid, n, call):
    RUN[call](pid, n)


# ---- a context over two shards ------------------------------------------------------------------
def test_sharded_context_takes_the_smallest_fault():
    """Context(..., devices=[0, 0]) splits a host call's words into two shards:
    `u` off in shard 0 and `v` off in shard 1 -- the smaller index wins -- and
    each of them alone."""
    R = rows("test", 3)
    ctx = _ctx("test", "multi")
    assert ctx.device_count == 2
    lo, hi, edge = 300, 900, -(-R.W // 2)
    assert lo < edge <= hi < R.W
    in0 = VC.single_fault(R.b, VC.U, lo, party=1)
    in1 = VC.single_fault(R.b, VC.V, hi, party=2)
    both = VC.Case("u_in_shard0_v_in_shard1", "E", in0.edits + in1.edits, lo, frozenset(), None)
    for c, want in ((both, lo), (in0, lo), (in1, hi)):
        e = VC.expect(R.b, c)
        assert e.ff == want and not e.changed
        y, ff = ctx.recombine_verify(R.host(c))
        assert ff == want and np.array_equal(y, R.y), c.name
        m, ff = ctx.mask_input(R.host(c), R.sec)
        assert ff == want and np.array_equal(m, R.m), c.name


# ---- the Python client -----------------------------------------------------------------------------
def test_client_mirror_reports_u_and_v_faults_with_the_reference_message():
    import amphora_amd as A
    from amphora_amd import client
    pid, n = "test", 2
    R = rows(pid, n, W_OBJECT)
    util = client.SecretShareUtil(_ctx(pid))
    faults = [VC.single_fault(R.b, VC.U, 70, party=1), VC.single_fault(R.b, VC.V, 255, party=0)]

    def message(c):
        y, r, v, w, u = VC.columns(R.b, c)
        e = VC.expect(R.b, c)
        assert e.ff == c.want_ff
        return O.verification_failure_message(R.pr.p, e.ff, y, r, u, v, w)

    def bodies(texts, sid):
        return [json.dumps(dict(zip(("secretId", "tags") + A._lib.ODO_FIELD_NAMES,
                                    [str(sid), []] + [t.decode() for t in party])), separators=(",", ":"))
                for party in texts]

    for c in faults:
        odos = [A.OutputDeliveryObject(*[f.tobytes() for f in o]) for o in R.host(c)]
        with pytest.raises(A.IntegrityVerificationException) as err:
            client.verify_output_delivery_objects(util, odos)
        assert str(err.value) == message(c), c.name
    honest = [A.OutputDeliveryObject(*[f.tobytes() for f in o]) for o in R.arrays]
    assert client.verify_output_delivery_objects(util, honest) == list(R.b.cols[VC.Y])
    sids = [uuid.UUID(int=77 + i) for i in range(3)]
    lists = [bodies(R.host_texts(faults[0]), sids[0]), bodies(R.texts, sids[1]), bodies(R.host_texts(faults[1]), sids[2])]
    got = client.verify_vss_json_batch(util, lists, sids)
    assert got[1] == (sids[1], [], list(R.b.cols[VC.Y]))
    for o, c in ((0, faults[0]), (2, faults[1])):
        assert isinstance(got[o], A.IntegrityVerificationException) and str(got[o]) == message(c), c.name
