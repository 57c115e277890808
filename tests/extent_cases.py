"""The memory contract of the C ABI (include/amphora.h): every array of every
entry point placed inside guard bands the test owns, inputs surrounded once
by zeros (S0) and once by bytes that change a verdict or an output if even
one of them is consumed (S1), and one table of calls (CALLS) that
tests/test_buffer_extents.py drives on the GPU.

For each call and case the table gives the arrays with their documented
extent and alignment class (the header line is cited in the entry), the
expected status, verdict words and outputs -- from the C oracle
(oracle/coracle), oracle/amphora_oracle.py, Python's base64 / json or Python
ints (tests/field_cases.py), never from another call into the library -- and
the call itself on raw addresses.  run_plan() then asserts

  P1  status, verdict words and output payloads equal the reference,
  P2  the bands of every output and verdict word are untouched,
  P3  every input (payload and bands) is unchanged,
  P4  S0 and S1 give identical statuses and outputs.

Importable without a GPU (tests/test_extent_harness.py runs the checks against
numpy stand-ins with one planted error each).  An ordinary module, not a
conftest.
"""
from __future__ import annotations

import base64
import ctypes as C
import functools
import json

import numpy as np

from oracle import amphora_oracle as O
from oracle import coracle
from tests import field_cases as FC

BAND = 256
NF = 0x7F7F7F7F7F7F7F7F
OK, E_VERIFY, E_LEN, E_PARAM = 0, 1, 2, 3
F_DEVICE = 1
# values the library uses as a blank, a sentinel or a default character: JSON
# whitespace, base64's 'A' (what positions past nchars decode as) and '=',
# the byte of AMPH_NO_FAILURE, and zero
FORBIDDEN = (0x00, 0x20, ord("A"), ord("="), 0x7F)


def band_pattern(start: int, n: int) -> np.ndarray:
    """Position-dependent fill: (i * 167 + 13) & 0xFF -- all 256 values in any
    256 consecutive positions, so a shifted or repeated copy differs -- with
    the FORBIDDEN values moved to their high-bit twins."""
    i = np.arange(start, start + n, dtype=np.int64)
    v = ((i * 167 + 13) & 0xFF).astype(np.uint8)
    v[np.isin(v, FORBIDDEN)] ^= 0x80
    return v


# ---- array kinds: default payload offset from a 256-aligned base, hostile bytes ----
WORD, REC24, SIGN, VERDICT, OFFS, BYTES, B64, JSONTXT, XCHG = (
    "word", "rec24", "sign", "verdict", "offsets", "bytes", "b64", "json", "xchg")
OFFSET = {WORD: 48,    # an odd multiple of 16: 16-aligned, not 32- or 256-aligned
          REC24: 8,    # 24-character records: 8-aligned
          SIGN: 2,     # sign bytes: k_xenc_* reads them as uint16_t
          VERDICT: 8, OFFS: 8,  # int64 / uint64 words: 8-aligned
          BYTES: 0, B64: 16, JSONTXT: 0, XCHG: 0}  # texts: the residue the case names
_XFRAG = b',{"a":1,"b":2}'
_FRAG = {WORD: b"\xff", SIGN: b"\xff", OFFS: b"\xff", BYTES: b"\xff", VERDICT: b"\xff",
         B64: b"!=\xff", REC24: b"!=\xff", JSONTXT: b',{"value":"'}


def _cycle(frag: bytes, n: int, end_aligned: bool) -> bytes:
    reps = frag * (n // len(frag) + 2)
    return reps[len(reps) - n:] if end_aligned else reps[:n]


def hostile(kind: str, nfront: int, nback: int):
    """(front, back) band bytes of an input of this kind in S1: 0xFF words
    (non-canonical, >= p: a consumed word breaks a MAC or shifts a sum; a
    consumed sign byte negates), '!' '=' 0xFF around base64 text (each a bad
    character inside nchars), record openers around MaskedInput text, and
    whole pairs plus a bare ':' touching both ends of exchange text."""
    if kind == XCHG:
        return (_cycle(_XFRAG, nfront - 1, True) + b":", b":" + _cycle(_XFRAG, nback - 1, False))
    f = _FRAG[kind]
    return _cycle(f, nfront, True), _cycle(f, nback, False)


class Guarded:
    """One array inside bands of at least BAND bytes on each side, in an Arena
    (device: one torch uint8 buffer; host: one numpy buffer).  The payload
    starts `offset` bytes past a 256-aligned address."""

    def __init__(self, arena, name, kind, n, offset, data, fill, start):
        self.arena, self.name, self.kind, self.n, self.offset = arena, name, kind, int(n), int(offset)
        assert 0 <= self.offset < 256 and start % 256 == 0
        self.start = start                        # of the region, in the arena
        self.lo = BAND + self.offset              # of the payload, in the region
        self.size = self.lo + self.n + BAND
        img = band_pattern(start, self.size)      # outputs: pattern throughout, the payload included
        if data is not None:
            d = np.frombuffer(bytes(data), np.uint8) if isinstance(data, (bytes, bytearray)) else \
                np.ascontiguousarray(data).view(np.uint8).reshape(-1)
            assert d.size == self.n, (name, d.size, self.n)
            img[self.lo:self.lo + self.n] = d
            if fill == "zeros":
                img[:self.lo] = 0
                img[self.lo + self.n:] = 0
            elif fill == "hostile":
                front, back = hostile(kind, self.lo, BAND)
                img[:self.lo] = np.frombuffer(front, np.uint8)
                img[self.lo + self.n:] = np.frombuffer(back, np.uint8)
        self.before = img
        self.after = None

    @property
    def ptr(self) -> int:
        return self.arena.base + self.start + self.lo

    @property
    def view(self) -> np.ndarray:
        """Host arenas: the live payload (what a callee given the pointer writes)."""
        return self.arena.buf[self.start + self.lo: self.start + self.lo + self.n]

    @property
    def region(self) -> np.ndarray:
        """Host arenas: the live region, bands included."""
        return self.arena.buf[self.start: self.start + self.size]

    def payload(self) -> bytes:
        return self.after[self.lo:self.lo + self.n].tobytes()

    def _first_diff(self, lo, hi):
        d = np.nonzero(self.after[lo:hi] != self.before[lo:hi])[0]
        return None if d.size == 0 else int(d[0]) + lo - self.lo  # relative to the payload

    def check_untouched(self):
        """Both bands byte for byte as they were filled."""
        for lo, hi in ((0, self.lo), (self.lo + self.n, self.size)):
            at = self._first_diff(lo, hi)
            assert at is None, "%s (%s, %d bytes): band byte at payload offset %d changed: 0x%02x -> 0x%02x" % (
                self.name, self.kind, self.n, at, self.before[self.lo + at], self.after[self.lo + at])

    def check_unchanged(self):
        """An input: payload and bands equal the bytes uploaded."""
        at = self._first_diff(0, self.size)
        assert at is None, "input %s (%s, %d bytes): byte at payload offset %d changed: 0x%02x -> 0x%02x" % (
            self.name, self.kind, self.n, at, self.before[self.lo + at], self.after[self.lo + at])


_DEV_BUF = {}


class Arena:
    """Every Guarded array of one call in one allocation the test owns: an
    overrun of any of them lands in a band (or a neighbour's band), never
    outside the allocation."""

    def __init__(self, device: bool):
        self.device, self.items, self.size = device, [], 0
        self.base = self.buf = self.t = None

    def add(self, name, kind, n=None, data=None, offset=None, fill="pattern") -> Guarded:
        if data is not None and n is None:
            n = len(data) if isinstance(data, (bytes, bytearray)) else np.asarray(data).nbytes
        g = Guarded(self, name, kind, n, OFFSET[kind] if offset is None else offset, data, fill, self.size)
        self.items.append(g)
        self.size += -(-g.size // 256) * 256
        return g

    def commit(self):
        img = np.zeros(self.size, np.uint8)
        for g in self.items:
            img[g.start:g.start + g.size] = g.before
        if self.device:
            import torch
            cap = 1 << 22
            while cap < self.size:
                cap *= 2
            if _DEV_BUF.get("cap", 0) < cap:
                _DEV_BUF["t"], _DEV_BUF["cap"] = torch.empty(cap, dtype=torch.uint8, device="cuda"), cap
            self.t = _DEV_BUF["t"][:self.size]
            self.base = self.t.data_ptr()
            self.t.copy_(torch.from_numpy(img))
        else:
            raw = np.zeros(self.size + 256, np.uint8)
            shift = -raw.ctypes.data % 256
            self.buf = raw[shift:shift + self.size]
            self.buf[:] = img
            self._raw, self.base = raw, raw.ctypes.data + shift
        assert self.base % 256 == 0
        return self

    def fetch(self):
        img = self.t.cpu().numpy() if self.device else self.buf.copy()
        for g in self.items:
            g.after = img[g.start:g.start + g.size]


def guard(kind, n=None, data=None, offset=None, fill="pattern", name="array") -> Guarded:
    """One host Guarded array in an arena of its own (stand-ins, unit tests)."""
    a = Arena(False)
    g = a.add(name, kind, n=n, data=data, offset=offset, fill=fill)
    a.commit()
    return g


# ---- a call's arrays and a case of it ------------------------------------------------
class Arr:
    """One array argument.  Inputs carry `data`.  Outputs carry `n` and what
    P1 expects of the payload: `expect` (bytes; a shorter value is compared
    with the payload's prefix, None = unspecified by the header) or `verdict`
    (an index or a list of them, -1 = none: AMPH_NO_FAILURE in a device word,
    -1 in a host word).  host=True: host memory in device mode too."""

    def __init__(self, name, kind, data=None, n=None, expect=None, verdict=None, offset=None, host=False,
                 value=None):
        self.name, self.kind, self.data, self.offset, self.host = name, kind, data, offset, host
        self.verdict, self.value = verdict, value
        if value is not None:  # a plain 8-byte word with the same value in both modes (out_len, out_bytes)
            n, expect = 8, int(value).to_bytes(8, "little")
        if verdict is not None:
            n = 8 * (len(verdict) if isinstance(verdict, (list, tuple)) else 1)
        self.n = n
        self.untouched = isinstance(expect, str) and expect == "untouched"  # the call must not write the array
        self.expect = None if expect is None or self.untouched else bytes(expect)

    def expected(self, device: bool):
        if self.verdict is None:
            return self.expect
        vs = self.verdict if isinstance(self.verdict, (list, tuple)) else [self.verdict]
        none = NF if (device and not self.host) else -1
        return b"".join(int(none if v < 0 else v).to_bytes(8, "little", signed=True) for v in vs)


class Plan:
    """One case of one call: call(L, h, p, flags, stream) -> status with
    p = {array name: address}; status = (device mode, host mode)."""

    def __init__(self, label, ins, outs, call, status=(OK, OK), check=None):
        self.label, self.ins, self.outs, self.call, self.status = label, ins, outs, call, status
        self.check = check  # check({name: whole output payload}): a reference that is a property of the outputs


SURROUNDS = (("S0", "zeros"), ("S1", "hostile"))


def check_plan(plan: "Plan", device: bool, st, ins, outs, where: str):
    """P1-P3 of one run whose arrays have been fetched (ins / outs = {name:
    Guarded} with `after` set); returns the outputs that have a reference."""
    want = plan.status[0 if device else 1]
    assert st == want, "%s: status %d, expected %d" % (where, st, want)             # P1
    got = {}
    for a in plan.outs:
        exp, pay = a.expected(device), outs[a.name].payload()
        if exp is not None:
            if pay[:len(exp)] != exp:
                at = next(i for i in range(len(exp)) if pay[i] != exp[i])
                raise AssertionError("%s: output %s differs from the reference at byte %d of %d: "
                                     "0x%02x, expected 0x%02x" % (where, a.name, at, len(exp), pay[at], exp[at]))
            got[a.name] = pay[:len(exp)]
        if a.untouched:
            g = outs[a.name]
            assert pay == g.before[g.lo:g.lo + g.n].tobytes(), "%s: output %s was written" % (where, a.name)
        try:
            outs[a.name].check_untouched()                                           # P2
        except AssertionError as e:
            raise AssertionError("%s: %s" % (where, e)) from None
    if plan.check:
        whole = {a.name: outs[a.name].payload() for a in plan.outs}
        plan.check(whole)
        got.update(whole)
    for a in plan.ins:
        try:
            ins[a.name].check_unchanged()                                            # P3
        except AssertionError as e:
            raise AssertionError("%s: %s" % (where, e)) from None
    return got


def run_plan(plan: Plan, device: bool, invoke, sync=None):
    """invoke(ins, outs) -> status, with ins / outs = {name: Guarded}.
    Asserts P1-P4; returns the S0 outputs."""
    seen = {}
    for sname, fill in SURROUNDS:
        main, aux = Arena(device), Arena(False)
        ins = {a.name: (aux if a.host else main).add(a.name, a.kind, data=a.data, offset=a.offset, fill=fill)
               for a in plan.ins}
        outs = {a.name: (aux if a.host else main).add(a.name, a.kind, n=a.n, offset=a.offset) for a in plan.outs}
        main.commit()
        aux.commit()
        st = invoke(ins, outs)
        if sync:
            sync()
        main.fetch()
        aux.fetch()
        got = check_plan(plan, device, st, ins, outs, "%s [%s]" % (plan.label, sname))
        seen[sname] = (st, got)
    s0, s1 = seen["S0"], seen["S1"]                                                      # P4
    assert s0[0] == s1[0], "%s: the status depends on the bytes around the inputs" % plan.label
    for k in s0[1]:
        assert s0[1][k] == s1[1][k], "%s: output %s depends on the bytes around the inputs" % (plan.label, k)
    return s0[1]


# ---- inputs and references, once per prime -------------------------------------------
LANE_SIZES = [1, 63, 64, 65, 1023, 1024, 1025]   # one word per lane, block 1024
STRIDE_SIZES = [191, 192, 193, 400]              # AMPH_BLOCK=64, AMPH_GRID_CAP=3: 192 lanes stride
PAIR_SIZES = [1, 127, 128, 129, 257]             # kPairBlock = 128
WIRE_SIZES = [1, 2, 3, 191, 192, 193, 385]       # 192 words per workgroup; 1, 2, 3: the padding shapes
JSON_SIZES = [0, 1, 127, 128, 129]
BULK_SIZES = [1, 2, 3, 3071, 3072, 3073]         # 12 * 256 bytes per block-kernel workgroup
BULK_OFFSETS = [0, 1, 15]
RECORD_SIZES = [1, 255, 256, 257]
XENC_SIZES = [1, 255, 256, 257, 1023, 1024, 1025]
XDEC_LENGTHS = [8191, 8192, 8193, 16383, 16384, 16385]  # kDecSpan = 8192
SESSION_SIZES = [1, 128, 129]
PARTIES = [1, 3, 5]   # templated, and the run-time form either side of the AMPH_DISPATCH_NP_SMALL* split
WMAX = 1025
PIDS = ["test", "m89"]


def le8(v, signed=False):
    return int(v).to_bytes(8, "little", signed=signed)


def i64(addr):
    return C.cast(C.c_void_p(addr), C.POINTER(C.c_int64))


def vps(addrs):
    return (C.c_void_p * max(1, len(addrs)))(*addrs)


def raw(a) -> bytes:
    return np.ascontiguousarray(a).tobytes()


def jackson(signed_pairs) -> bytes:
    return json.dumps([{"a": a, "b": b} for a, b in signed_pairs], separators=(",", ":")).encode()


def data_text(words16) -> bytes:
    return json.dumps([{"value": base64.b64encode(bytes(w)).decode()} for w in words16],
                      separators=(",", ":")).encode()


class Data:
    """One prime's inputs at the largest size and the oracle's field; every
    operation here is word by word, so a prefix of W words is the case for W."""

    def __init__(self, pid):
        self.pr = FC.BY_ID[pid]
        self.F = coracle.Field(self.pr.p, self.pr.r, self.pr.rinv, threads=4)
        self.secrets = self.F.synth_words(seed=5, count=WMAX, mont=False)
        self.secrets[::5] = 0xFF  # raw 128-bit integers >= p
        self.key = (FC.UNIFORM_WORDS[1] % (self.pr.p - 1)) + 1

    @functools.lru_cache(maxsize=None)
    def odos(self, n):
        od, _ = self.F.synth_odos(seed=7000 + n, n=n, W=WMAX, noncanon_permille=200)
        return [tuple(np.ascontiguousarray(f) for f in o) for o in od]

    def odo_prefix(self, n, W, fault=None, lo=0):
        od = [tuple(f[lo:lo + W].copy() for f in o) for o in self.odos(n)]
        return FC.with_fault(od, fault) if fault is not None else od

    @functools.lru_cache(maxsize=None)
    def columns(self, n):
        """The canonical y, r, v, w, u columns of odos(n) (the C oracle's recombine)."""
        return [self.F.recombine([o[k] for o in self.odos(n)]) for k in range(5)]

    @functools.lru_cache(maxsize=None)
    def ints(self, what):
        sec = FC.ints(self.secrets)
        if what == "to_gfp":
            return FC.arr([FC.to_gfp(self.pr, x % self.pr.p) for x in sec])
        if what == "from_gfp":
            return FC.arr([FC.from_gfp(self.pr, x) for x in sec])
        assert what == "mask_words"
        return FC.arr(FC.mask_words(self.pr, sec, FC.ints(self.columns(3)[0])))

    @functools.lru_cache(maxsize=None)
    def party(self, j, W=257):
        """Party j's share data (W, 32), 2 W masks (32 B) and 2 W triples (96 B)."""
        F = self.F
        return (F.synth_words(seed=100 + j, count=2 * W).reshape(W, 32),
                F.synth_words(seed=200 + j, count=4 * W).reshape(2 * W, 32),
                F.synth_words(seed=300 + j, count=12 * W).reshape(2 * W, 96))

    def pre(self, j, W, stride=32):
        sh, mk, tr = self.party(j)
        share = np.ascontiguousarray(sh[:W, :stride])
        return share, mk[:2 * W], tr[:2 * W], self.F.odo_pre(share, stride, mk[:2 * W], tr[:2 * W])

    def pre_text(self, j, W) -> bytes:
        _, _, _, (_, _, _, mag, neg) = self.pre(j, W)
        return jackson(FC.signed_of(mag, neg))


@functools.lru_cache(maxsize=None)
def data(pid) -> Data:
    return Data(pid)


FIELD = "yrvwu"


def odo_arrs(od, kind=WORD):
    return [Arr("%s%d" % (FIELD[k], j), kind, data=o[k]) for j, o in enumerate(od) for k in range(5)]


def odo_struct(p, n, nbytes):
    from amphora_amd import _lib
    arr = (_lib._AmphOdo * n)()
    for j in range(n):
        arr[j] = _lib._AmphOdo(*[p["%s%d" % (f, j)] for f in FIELD], nbytes)
    return arr


def b64_struct(p, n, nchars):
    from amphora_amd import _lib
    arr = (_lib._AmphOdoB64 * n)()
    for j in range(n):
        arr[j] = _lib._AmphOdoB64(*[p["%s%d" % (f, j)] for f in FIELD], nchars)
    return arr


def texts_of(od):
    return [tuple(np.frombuffer(base64.b64encode(raw(f)), np.uint8) for f in o) for o in od]


def lane_sizes(strided):
    return STRIDE_SIZES if strided else LANE_SIZES


# ---- the calls -----------------------------------------------------------------------
# Every generator yields Plans.  `strided` selects the sizes of the context
# created under AMPH_BLOCK=64 / AMPH_GRID_CAP=3 (one-word-per-lane kernels only).
def g_recombine_verify(d, strided=False):
    for n in PARTIES:
        for W in lane_sizes(strided):
            for fault in (None, W - 1):
                od = d.odo_prefix(n, W, fault)
                y, ff = d.F.recombine_verify(od)
                assert ff == (-1 if fault is None else fault)
                yield Plan("recombine_verify n=%d W=%d fault=%s" % (n, W, fault), odo_arrs(od),
                           [Arr("out", WORD, n=16 * W, expect=raw(y)), Arr("ff", VERDICT, verdict=ff)],
                           lambda L, h, p, fl, s, n=n, W=W: L.amph_recombine_verify(
                               h, odo_struct(p, n, 16 * W), n, p["out"], i64(p["ff"]), fl, s),
                           (OK, OK if fault is None else E_VERIFY))


def g_mask_input(d, strided=False):
    for n in PARTIES:
        for W in lane_sizes(strided):
            # every mask word masked; then a verify-only tail (WRITE_Y = false) that holds the fault
            for S, fault in ((W, None), (W - 3 if W > 3 else W, W - 1)):
                od = d.odo_prefix(n, W, fault)
                sec = d.secrets[:S]
                m, _ = d.F.mask_input(sec, [tuple(f[:S] for f in o) for o in od])
                _, ff = d.F.recombine_verify(od)
                assert ff == (-1 if fault is None else fault)
                # the header promises the masked words of a call that verified
                yield Plan("mask_input n=%d W=%d S=%d fault=%s" % (n, W, S, fault),
                           odo_arrs(od) + [Arr("secrets", WORD, data=sec)],
                           [Arr("out", WORD, n=16 * S, expect=raw(m) if fault is None else None),
                            Arr("ff", VERDICT, verdict=ff)],
                           lambda L, h, p, fl, s, n=n, W=W, S=S: L.amph_mask_input(
                               h, odo_struct(p, n, 16 * W), n, p["secrets"], S, p["out"], i64(p["ff"]), fl, s),
                           (OK, OK if fault is None else E_VERIFY))


def packed_offsets(T):
    """Empty objects first, last and adjacent."""
    a, b = T // 3, (2 * T + 2) // 3
    return [0, 0, a, a, a, b, T, T]


def _g_packed(d, masked, strided):
    for n in PARTIES:
        for T in lane_sizes(strided):
            offs = packed_offsets(T)
            K = len(offs) - 1
            last = max(o for o in range(K) if offs[o + 1] > offs[o])
            for faults in ((), (0, offs[last + 1] - 1)):  # word 0; the last word of the last non-empty object
                od = d.odo_prefix(n, T)
                for at in set(faults):
                    od = FC.with_fault(od, at)
                y, _ = d.F.recombine_verify(od)
                verdicts = []
                for o in range(K):  # the oracle's verdict on each object alone
                    lo, hi = offs[o], offs[o + 1]
                    verdicts.append(-1 if hi == lo else
                                    d.F.recombine_verify([tuple(f[lo:hi] for f in p_) for p_ in od])[1])
                assert (max(verdicts) >= 0) == bool(faults)
                ins = odo_arrs(od) + [Arr("offsets", OFFS, data=np.array(offs, np.uint64))]
                if masked:
                    sec = d.secrets[:T]
                    exp, _ = d.F.mask_input(sec, od)
                    ins.append(Arr("secrets", WORD, data=sec))
                    call = lambda L, h, p, fl, s, n=n, T=T, K=K: L.amph_mask_input_packed(  # noqa: E731
                        h, odo_struct(p, n, 16 * T), n, p["offsets"], K, p["secrets"], p["out"], p["ff"], fl, s)
                else:
                    exp = y
                    call = lambda L, h, p, fl, s, n=n, T=T, K=K: L.amph_recombine_verify_packed(  # noqa: E731
                        h, odo_struct(p, n, 16 * T), n, p["offsets"], K, p["out"], p["ff"], fl, s)
                yield Plan("%s_packed n=%d T=%d faults=%s" % ("mask_input" if masked else "recombine_verify", n, T,
                                                               faults), ins,
                           [Arr("out", WORD, n=16 * T, expect=raw(exp)),  # written for failed objects too
                            Arr("ff", VERDICT, verdict=verdicts)], call, (OK, E_VERIFY if faults else OK))


def g_recombine_verify_packed(d, strided=False):
    return _g_packed(d, False, strided)


def g_mask_input_packed(d, strided=False):
    return _g_packed(d, True, strided)


def g_recombine(d, strided=False):
    for n in PARTIES:
        for W in lane_sizes(strided):
            sh = [o[0][:W] for o in d.odos(n)]
            exp = d.F.recombine(sh)
            yield Plan("recombine n=%d W=%d" % (n, W), [Arr("s%d" % j, WORD, data=x) for j, x in enumerate(sh)],
                       [Arr("out", WORD, n=16 * W, expect=raw(exp))],
                       lambda L, h, p, fl, s, n=n, W=W: L.amph_recombine(
                           h, vps([p["s%d" % j] for j in range(n)]), n, 16 * W, p["out"], fl, s))


def g_recombine_object(d, strided=False):
    for n in PARTIES:
        for W in lane_sizes(strided):
            full = [raw(o[1][:W]) for o in d.odos(n)]
            sh = list(full)
            if n >= 2:  # a longer party (cut to W words) and one ending inside word W - 1 (zero-padded)
                sh[1] = full[1] + b"\xEE" * 16
            if n >= 3:
                sh[n - 1] = full[n - 1][:16 * W - 8]
            exp = d.F.recombine_object(sh)
            lens = [len(x) for x in sh]
            yield Plan("recombine_object n=%d W=%d" % (n, W),
                       [Arr("s%d" % j, WORD, data=x) for j, x in enumerate(sh)],
                       [Arr("out", WORD, n=16 * W, expect=raw(exp))],
                       lambda L, h, p, fl, s, n=n, lens=lens: L.amph_recombine_object(
                           h, vps([p["s%d" % j] for j in range(n)]), n, (C.c_size_t * n)(*lens), p["out"], fl, s))


def g_verify(d, strided=False):
    n = 3
    y, r, v, w, u = d.columns(n)
    p_ = d.pr.p
    for W in lane_sizes(strided):
        for fault in (None, W - 1):
            ww = w[:W].copy()
            if fault is not None:
                ww[fault] = FC.arr([(FC.ints(ww[fault:fault + 1])[0] + 1) % p_])[0]
            cols = [y[:W], r[:W], u[:W], v[:W], ww]
            ff = O.first_failing_index(p_, *[FC.ints(c) for c in cols])
            assert ff == (-1 if fault is None else fault)
            yield Plan("verify W=%d fault=%s" % (W, fault),
                       [Arr(k, WORD, data=c) for k, c in zip(("y", "r", "u", "v", "w"), cols)],
                       [Arr("ff", VERDICT, verdict=ff)],
                       lambda L, h, p, fl, s, W=W: L.amph_verify(h, p["y"], p["r"], p["u"], p["v"], p["w"], W,
                                                                 i64(p["ff"]), fl, s),
                       (OK, OK if fault is None else E_VERIFY))


def g_mask_words(d, strided=False):
    masks = d.columns(3)[0]
    for W in lane_sizes(strided):
        yield Plan("mask_words W=%d" % W, [Arr("secrets", WORD, data=d.secrets[:W]), Arr("masks", WORD, data=masks[:W])],
                   [Arr("out", WORD, n=16 * W, expect=raw(d.ints("mask_words")[:W]))],
                   lambda L, h, p, fl, s, W=W: L.amph_mask_words(h, p["secrets"], p["masks"], W, p["out"], fl, s))


def _g_gfp(d, name, strided):
    for W in lane_sizes(strided):
        yield Plan("%s W=%d" % (name, W), [Arr("in", WORD, data=d.secrets[:W])],
                   [Arr("out", WORD, n=16 * W, expect=raw(d.ints(name)[:W]))],
                   lambda L, h, p, fl, s, W=W: getattr(L, "amph_" + name)(h, p["in"], W, p["out"], fl, s))


def g_to_gfp(d, strided=False):
    return _g_gfp(d, "to_gfp", strided)


def g_from_gfp(d, strided=False):
    return _g_gfp(d, "from_gfp", strided)


def g_convert_share(d):
    masked = d.secrets[:257]
    tup = d.party(0)[1][:257]
    key = d.key
    for W in PAIR_SIZES:
        for uz in (0, 1):
            exp = d.F.convert_share(np.ascontiguousarray(masked[:W]), np.ascontiguousarray(tup[:W]), key, bool(uz))
            yield Plan("convert_share W=%d uz=%d" % (W, uz),
                       [Arr("masked", WORD, data=masked[:W]), Arr("tuples", WORD, data=tup[:W])],
                       [Arr("out", WORD, n=32 * W, expect=raw(exp))],
                       lambda L, h, p, fl, s, W=W, uz=uz: L.amph_convert_share(
                           h, p["masked"], p["tuples"], W, FC.arr([key])[0].tobytes(), uz, p["out"], fl, s))


def g_odo_pre(d):
    for stride in (16, 32):
        for W in PAIR_SIZES:
            share, mk, tr, (y, r, v, mag, neg) = d.pre(0, W, stride)
            yield Plan("odo_pre stride=%d W=%d" % (stride, W),
                       [Arr("share", WORD, data=share), Arr("masks", WORD, data=mk), Arr("triples", WORD, data=tr)],
                       [Arr("y", WORD, n=16 * W, expect=raw(y)), Arr("r", WORD, n=16 * W, expect=raw(r)),
                        Arr("v", WORD, n=16 * W, expect=raw(v)), Arr("mag", WORD, n=64 * W, expect=raw(mag)),
                        Arr("neg", SIGN, n=4 * W, expect=raw(neg))],
                       lambda L, h, p, fl, s, W=W, stride=stride: L.amph_odo_pre(
                           h, p["share"], stride, p["masks"], p["triples"], W, p["y"], p["r"], p["v"], p["mag"],
                           p["neg"], fl, s))


def _diffs(d, n, W):
    pres = [d.pre(j, W)[3] for j in range(n)]
    return [x[3] for x in pres], [x[4] for x in pres]


def _diff_arrs(mags, negs):
    return [Arr("mag%d" % j, WORD, data=m) for j, m in enumerate(mags)] + \
           [Arr("neg%d" % j, SIGN, data=g) for j, g in enumerate(negs)]


def g_open_diffs(d):
    for n in PARTIES:
        for W in PAIR_SIZES:
            mags, negs = _diffs(d, n, W)
            exp = d.F.recombine_diffs(mags, negs)
            yield Plan("open_diffs n=%d W=%d" % (n, W), _diff_arrs(mags, negs),
                       [Arr("out", WORD, n=64 * W, expect=raw(exp))],
                       lambda L, h, p, fl, s, n=n, W=W: L.amph_open_diffs(
                           h, vps([p["mag%d" % j] for j in range(n)]), vps([p["neg%d" % j] for j in range(n)]), n,
                           2 * W, p["out"], fl, s))


def g_odo_post(d):
    for W in PAIR_SIZES:
        mags, negs = _diffs(d, 3, W)
        opened = d.F.recombine_diffs(mags, negs)
        tr = d.party(0)[2][:2 * W]
        for p0 in (1, 0):
            ew, eu = d.F.odo_post(opened.reshape(2 * W, 32), np.ascontiguousarray(tr), bool(p0))
            yield Plan("odo_post W=%d p0=%d" % (W, p0), [Arr("opened", WORD, data=opened), Arr("triples", WORD, data=tr)],
                       [Arr("w", WORD, n=16 * W, expect=raw(ew)), Arr("u", WORD, n=16 * W, expect=raw(eu))],
                       lambda L, h, p, fl, s, W=W, p0=p0: L.amph_odo_post(h, p["opened"], p["triples"], W, p0, p["w"],
                                                                          p["u"], fl, s))


def g_open_post(d):
    for n in PARTIES:
        for W in PAIR_SIZES:
            mags, negs = _diffs(d, n, W)
            opened = d.F.recombine_diffs(mags, negs)
            tr = d.party(0)[2][:2 * W]
            p0 = n % 2
            ew, eu = d.F.odo_post(opened.reshape(2 * W, 32), np.ascontiguousarray(tr), bool(p0))
            yield Plan("open_post n=%d W=%d" % (n, W), _diff_arrs(mags, negs) + [Arr("triples", WORD, data=tr)],
                       [Arr("w", WORD, n=16 * W, expect=raw(ew)), Arr("u", WORD, n=16 * W, expect=raw(eu))],
                       lambda L, h, p, fl, s, n=n, W=W, p0=p0: L.amph_open_post(
                           h, vps([p["mag%d" % j] for j in range(n)]), vps([p["neg%d" % j] for j in range(n)]), n,
                           p["triples"], W, p0, p["w"], p["u"], fl, s))


def _bulk(nb):
    return np.random.default_rng(nb).integers(0, 256, nb, dtype=np.uint8).tobytes()


def g_base64_encode(d):
    for nb in BULK_SIZES:
        rawb = _bulk(nb)
        exp = base64.b64encode(rawb)
        for off in BULK_OFFSETS:
            yield Plan("base64_encode nbytes=%d offset=%d" % (nb, off), [Arr("in", BYTES, data=rawb, offset=off)],
                       [Arr("out", B64, n=len(exp), expect=exp, offset=off)],
                       lambda L, h, p, fl, s, nb=nb: L.amph_base64_encode(h, p["in"], nb, p["out"], fl, s))


def g_base64_decode(d):
    """The output's extent is the decoded length: a clean padded text writes no
    byte past it (tests/test_wire.py pins the same)."""
    for nb in BULK_SIZES:
        rawb = _bulk(nb)
        text = base64.b64encode(rawb)
        for off in BULK_OFFSETS:
            for with_len in (False, True):
                outs = [Arr("out", BYTES, n=nb, expect=rawb, offset=off), Arr("bad", VERDICT, verdict=-1)]
                if with_len:  # a host size_t in both modes (device mode reads the padding back to set it)
                    outs.append(Arr("len", VERDICT, value=nb, host=True))
                yield Plan("base64_decode nbytes=%d offset=%d out_bytes=%s" % (nb, off, with_len),
                           [Arr("in", B64, data=text, offset=off)], outs,
                           lambda L, h, p, fl, s, nc=len(text), with_len=with_len: L.amph_base64_decode(
                               h, p["in"], nc, p["out"],
                               C.cast(C.c_void_p(p["len"]), C.POINTER(C.c_size_t)) if with_len else None,
                               i64(p["bad"]), fl, s))


def g_base64_encode_words(d):
    for W in RECORD_SIZES:
        exp = b"".join(base64.b64encode(raw(w)) for w in d.secrets[:W])
        yield Plan("base64_encode_words W=%d" % W, [Arr("in", WORD, data=d.secrets[:W])],
                   [Arr("out", REC24, n=24 * W, expect=exp)],
                   lambda L, h, p, fl, s, W=W: L.amph_base64_encode_words(h, p["in"], W, p["out"], fl, s))


def g_base64_decode_words(d):
    for W in RECORD_SIZES:
        text = b"".join(base64.b64encode(raw(w)) for w in d.secrets[:W])
        yield Plan("base64_decode_words W=%d" % W, [Arr("in", REC24, data=text)],
                   [Arr("out", WORD, n=16 * W, expect=raw(d.secrets[:W])), Arr("bad", VERDICT, verdict=-1)],
                   lambda L, h, p, fl, s, W=W: L.amph_base64_decode_words(h, p["in"], W, p["out"], i64(p["bad"]), fl, s))


def g_recombine_verify_b64(d):
    for n in PARTIES:
        for W in WIRE_SIZES:
            for fault in (None, W - 1):
                od = d.odo_prefix(n, W, fault)
                y, ff = d.F.recombine_verify(od)
                tx = texts_of(od)
                nchars = tx[0][0].size
                assert nchars == 4 * ((16 * W + 2) // 3)
                yield Plan("recombine_verify_b64 n=%d W=%d fault=%s" % (n, W, fault), odo_arrs(tx, B64),
                           [Arr("out", WORD, n=16 * W, expect=raw(y)), Arr("ff", VERDICT, verdict=ff),
                            Arr("bad", VERDICT, verdict=-1)],
                           lambda L, h, p, fl, s, n=n, W=W, nchars=nchars: L.amph_recombine_verify_b64(
                               h, b64_struct(p, n, nchars), n, W, p["out"], i64(p["ff"]), i64(p["bad"]), fl, s),
                           (OK, OK if fault is None else E_VERIFY))


def _mask_b64_plan(d, n, W, S, fault, want16, want24, label, status, bad_at=None):
    od = d.odo_prefix(n, W, fault)
    tx = [list(t) for t in texts_of(od)]
    nchars = tx[0][0].size
    bad = -1
    if bad_at is not None:  # party n - 1's r field
        t = tx[n - 1][1].copy()
        t[bad_at] = ord("*")
        tx[n - 1][1] = t
        bad = (5 * (n - 1) + 1) * nchars + bad_at
    sec = d.secrets[:S]
    clean = fault is None and bad_at is None and S <= W
    rest = "untouched" if S > W else None  # n_secrets > words: neither output array is written (amphora.h)
    outs = []
    if clean:
        m, _ = d.F.mask_input(sec, [tuple(f[:S] for f in o) for o in od])
    if want16:
        outs.append(Arr("o16", WORD, n=16 * S, expect=raw(m) if clean else rest))
    if want24:  # device: 16-byte aligned (amphora.h, amph_mask_input_b64)
        outs.append(Arr("o24", REC24, n=24 * S, offset=OFFSET[WORD],
                        expect=b"".join(base64.b64encode(raw(w)) for w in m) if clean else rest))
    _, ff = d.F.recombine_verify(od)
    outs += [Arr("ff", VERDICT, verdict=ff) if bad_at is None else Arr("ff", VERDICT, n=8),
             Arr("bad", VERDICT, verdict=bad)]
    return Plan(label, odo_arrs(tx, B64) + [Arr("secrets", WORD, data=sec)], outs,
                lambda L, h, p, fl, s: L.amph_mask_input_b64(
                    h, b64_struct(p, n, nchars), n, W, p["secrets"], S, p.get("o16"), p.get("o24"), i64(p["ff"]),
                    i64(p["bad"]), fl, s), status)


def g_mask_input_b64(d):
    for n in PARTIES:
        for W in WIRE_SIZES:
            for k, (want16, want24) in enumerate(((1, 1), (1, 0), (0, 1), (0, 0))):
                fault = None if k % 2 == 0 else W - 1
                S = W if k < 2 or W <= 3 else W - 3
                yield _mask_b64_plan(d, n, W, S, fault, want16, want24,
                                     "mask_input_b64 n=%d W=%d S=%d fault=%s o16=%d o24=%d" % (n, W, S, fault, want16,
                                                                                             want24),
                                     (OK, OK if fault is None else E_VERIFY))


def g_mask_input_b64_more_secrets(d):
    """n_secrets > words: the texts decode and every mask verifies first, then
    AMPH_E_LEN; device mode waits for the verdicts, so the statuses are the
    host's (amphora.h, amph_mask_input_b64)."""
    n, W, S = 2, 8, 10
    for want16, want24 in ((1, 1), (1, 0), (0, 1)):
        yield _mask_b64_plan(d, n, W, S, None, want16, want24, "mask_input_b64 S>W honest W=8 o16=%d o24=%d" % (want16, want24), (E_LEN, E_LEN))
        yield _mask_b64_plan(d, n, W, S, 5, want16, want24, "mask_input_b64 S>W MAC fault W=8 o16=%d o24=%d" % (want16, want24), (E_VERIFY, E_VERIFY))
        yield _mask_b64_plan(d, n, W, S, None, want16, want24, "mask_input_b64 S>W bad character W=8 o16=%d o24=%d" % (want16, want24),
                             (E_PARAM, E_PARAM), bad_at=17)


def g_mask_input_json(d):
    n = 3
    for W in JSON_SIZES:
        for fault in (None,) if W == 0 else (None, W - 1):
            od = d.odo_prefix(n, W, fault)
            tx = texts_of(od)
            nchars = tx[0][0].size
            sec = d.secrets[:W]
            m, _ = d.F.mask_input(sec, od) if W else (np.zeros((0, 16), np.uint8), -1)
            ff = -1 if fault is None else fault
            text = data_text(m)
            assert len(text) == (37 * W + 1 if W else 2)
            yield Plan("mask_input_json W=%d fault=%s" % (W, fault), odo_arrs(tx, B64) + [Arr("secrets", WORD, data=sec)],
                       [Arr("text", JSONTXT, n=len(text), offset=OFFSET[B64], expect=text if fault is None else None),
                        Arr("ff", VERDICT, verdict=ff), Arr("bad", VERDICT, verdict=-1)],
                       lambda L, h, p, fl, s, W=W, nchars=nchars, cap=len(text): L.amph_mask_input_json(
                           h, b64_struct(p, n, nchars), n, W, p["secrets"], W, p["text"], cap, i64(p["ff"]),
                           i64(p["bad"]), fl, s),
                       (OK, OK if fault is None else E_VERIFY))


def g_convert_share_json(d):
    masked = d.secrets[:129]
    tup = d.party(0)[1][:129]
    key = d.key
    for W in JSON_SIZES:
        text = data_text(masked[:W])
        for k, off in enumerate(BULK_OFFSETS):
            uz = k % 2
            exp = d.F.convert_share(np.ascontiguousarray(masked[:W]), np.ascontiguousarray(tup[:W]), key, bool(uz)) \
                if W else np.zeros((0, 32), np.uint8)
            for bad in (None,) if W == 0 else (None, len(text) - 1):  # the final ']' replaced
                t = bytearray(text)
                if bad is not None:
                    t[bad] = ord(",")
                # out_share is unspecified when bad_index reports a failure (amphora.h, amph_convert_share_json)
                yield Plan("convert_share_json W=%d offset=%d bad=%s" % (W, off, bad),
                           [Arr("text", JSONTXT, data=bytes(t), offset=off), Arr("tuples", WORD, data=tup[:W])],
                           [Arr("out", WORD, n=32 * W, expect=raw(exp) if bad is None else None),
                            Arr("bad", VERDICT, verdict=-1 if bad is None else bad)],
                           lambda L, h, p, fl, s, W=W, uz=uz, ln=len(text): L.amph_convert_share_json(
                               h, p["text"], ln, W, p["tuples"], FC.arr([key])[0].tobytes(), uz, p["out"],
                               i64(p["bad"]), fl, s),
                           (OK, OK if bad is None else E_PARAM))


def exchange_values(kind, npairs):
    """2 * npairs (magnitude, negative flag) values of one magnitude set."""
    if kind == "zero":      # 13-byte entries: one pair alone is shorter than one 16-byte unit
        return [(0, 0)] * (2 * npairs)
    if kind == "max":       # 92-byte entries
        return [(FC.MASK128, 1)] * (2 * npairs)
    vals = []
    for k in range(2 * npairs):  # 1..39 digits cycling, mixed signs, negative zero
        L = 1 + k % 39
        v = k % 10 if L == 1 else 10 ** (L - 1) + (k * 7919) % (10 ** (L - 1))
        vals.append((v, 1 if k % 3 == 0 else 0))
    assert vals[0] == (0, 1) and max(v for v, _ in vals) <= FC.MASK128
    return vals


@functools.lru_cache(maxsize=None)
def exchange_case(kind, npairs):
    vals = exchange_values(kind, npairs)
    mag = FC.arr([v for v, _ in vals])
    neg = np.array([g for _, g in vals], np.uint8)
    signed = [-v if g else v for v, g in vals]
    return mag, neg, jackson(list(zip(signed[0::2], signed[1::2])))


def g_exchange_encode(d):
    """out from *out_len to out_cap is unspecified (amphora.h says so): the
    text is compared up to out_len, the bands start at out_cap."""
    for kind in ("zero", "max", "mixed"):
        for P in XENC_SIZES:
            mag, neg, text = exchange_case(kind, P)
            cap = 92 * P + 2
            for align in range(16):
                yield Plan("exchange_encode %s npairs=%d align=%d" % (kind, P, align),
                           [Arr("mag", WORD, data=mag), Arr("neg", SIGN, data=neg)],
                           [Arr("out", XCHG, n=cap, expect=text, offset=align), Arr("len", VERDICT, value=len(text))],
                           lambda L, h, p, fl, s, P=P, cap=cap: L.amph_exchange_encode(
                               h, p["mag"], p["neg"], P, p["out"], cap, p["len"], fl, s))


@functools.lru_cache(maxsize=None)
def decode_text(length):
    """A compact mixed-set text brought to `length` bytes by spaces before ']'."""
    P = 1
    while len(exchange_case("mixed", P + 1)[2]) <= length:
        P += 1
    mag, neg, text = exchange_case("mixed", P)
    text = text[:-1] + b" " * (length - len(text)) + b"]"
    assert len(text) == length
    # the decoder's sign byte: 1 = negative as written ("-0" does not occur in a text)
    vals = exchange_values("mixed", P)
    neg = np.array([1 if g and v else 0 for v, g in vals], np.uint8)
    return P, mag, neg, text


def g_exchange_decode(d):
    cases = [(ln, a) for ln in XDEC_LENGTHS for a in BULK_OFFSETS] + [(0, a) for a in range(16)]
    for ln, align in cases:
        if ln == 0:  # one 13-byte pair: with its brackets shorter than one 16-byte chunk
            P, mag, neg, text = 1, FC.arr([7, 0]), np.zeros(2, np.uint8), b'[{"a":7,"b":0}]'
            ln = len(text)
        else:
            P, mag, neg, text = decode_text(ln)
        yield Plan("exchange_decode len=%d align=%d" % (ln, align), [Arr("text", XCHG, data=text, offset=align)],
                   [Arr("mag", WORD, n=32 * P, expect=raw(mag)), Arr("neg", SIGN, n=2 * P, expect=raw(neg)),
                    Arr("bad", VERDICT, verdict=-1)],
                   lambda L, h, p, fl, s, P=P, ln=ln: L.amph_exchange_decode(h, p["text"], ln, P, p["mag"], p["neg"],
                                                                             i64(p["bad"]), fl, s))


# -- device-only generators ------------------------------------------------------------
def g_synth_odos(d, strided=False):
    """The reference is the oracle's verdict on what was generated: the fields
    recombine to out_plain_y and fail exactly at fault_index."""
    for n in PARTIES:
        for W in lane_sizes(strided):
            fault = W - 1 if W % 2 else -1
            names = ["%s%d" % (FIELD[k], j) for k in range(5) for j in range(n)]

            def check(got, n=n, W=W, fault=fault):
                od = [tuple(np.frombuffer(got["%s%d" % (f, j)], np.uint8).reshape(W, 16) for f in FIELD)
                      for j in range(n)]
                y, ff = d.F.recombine_verify(od)
                assert ff == fault, ("synth_odos", n, W, ff)
                assert raw(y) == got["plain"]
                assert all(x < d.pr.p for x in FC.ints(np.frombuffer(got["plain"], np.uint8)))
            yield Plan("synth_odos n=%d W=%d fault=%d" % (n, W, fault), [],
                       [Arr(nm, WORD, n=16 * W) for nm in names] + [Arr("plain", WORD, n=16 * W)],
                       lambda L, h, p, fl, s, n=n, W=W, fault=fault, names=names: L.amph_synth_odos(
                           h, 77 + n, n, W, vps([p[nm] for nm in names]), p["plain"], fault, 100, s), check=check)


def g_synth_words(d, strided=False):
    for W in lane_sizes(strided):
        exp = d.F.synth_words(seed=9, count=W, mont=False)
        yield Plan("synth_words count=%d" % W, [], [Arr("out", WORD, n=16 * W, expect=raw(exp))],
                   lambda L, h, p, fl, s, W=W: L.amph_synth_words(h, 9, W, p["out"], s))


def g_stream_probe(d, strided=False):
    for n in PARTIES:
        for W in lane_sizes(strided):
            od = d.odo_prefix(n, W)
            x = d.secrets[:W].copy()
            for o in od:
                for f in o:
                    x ^= f
            yield Plan("stream_probe n=%d W=%d" % (n, W), odo_arrs(od) + [Arr("secrets", WORD, data=d.secrets[:W])],
                       [Arr("out", WORD, n=16 * W, expect=raw(x))],
                       lambda L, h, p, fl, s, n=n, W=W: L.amph_stream_probe(h, odo_struct(p, n, 16 * W), n,
                                                                            p["secrets"], W, p["out"], s))


def _session_expect(d, n, W, p0=True):
    pres = [d.pre(j, W)[3] for j in range(n)]
    opened = d.F.recombine_diffs([x[3] for x in pres], [x[4] for x in pres])
    ow, ou = d.F.odo_post(opened.reshape(2 * W, 32), np.ascontiguousarray(d.party(0)[2][:2 * W]), p0)
    return pres[0], ow, ou


def _read_dev(ptr, n, device=0):
    from amphora_amd import _lib
    return _lib._dev_view(ptr, n, "|u1", device).cpu().numpy().tobytes() if n else b""


def g_party_dev(d):
    """amph_party_begin_dev / _partner_dev / _finish_b64_dev: party 0 of n, the
    partners' texts (Jackson's text of the oracle's diffs) at odd residues."""
    for n in (2, 3):
        for W in SESSION_SIZES:
            share, mk, tr, _ = d.pre(0, W)
            (y, r, v, mag, neg), ow, ou = _session_expect(d, n, W)
            own = jackson(FC.signed_of(mag, neg))
            texts = [d.pre_text(j, W) for j in range(1, n)]
            fields = [base64.b64encode(raw(x)) for x in (y, r, v, ow, ou)]

            def call(L, h, p, fl, s, n=n, W=W, own=own, texts=texts, fields=fields):
                import torch
                ph = C.c_void_p()
                st = L.amph_party_begin_dev(h, p["share"], 32, p["masks"], p["triples"], W, n, p["y"], p["r"], p["v"],
                                            s, C.byref(ph))
                if st:
                    return st
                try:
                    for k, t in enumerate(texts, start=1):
                        st = L.amph_party_partner_dev(ph, k, p["text%d" % k], len(t), p["bad%d" % k], s)
                        if st:
                            return st
                    out = (C.c_void_p * 5)()
                    st = L.amph_party_finish_b64_dev(ph, 1, out, s)
                    if st:
                        return st
                    tp, lp = C.c_void_p(), C.c_void_p()
                    st = L.amph_party_text_dev(ph, C.byref(tp), C.byref(lp))
                    if st:
                        return st
                    torch.cuda.synchronize()
                    ln = int.from_bytes(_read_dev(lp.value, 8), "little")
                    assert ln == len(own) and _read_dev(tp.value, ln) == own, "the session's own text"
                    for k in range(5):
                        assert _read_dev(out[k], len(fields[k])) == fields[k], "field %d" % k
                finally:
                    L.amph_party_free(ph)
                return OK
            yield Plan("party_dev n=%d W=%d" % (n, W),
                       [Arr("share", WORD, data=share), Arr("masks", WORD, data=mk), Arr("triples", WORD, data=tr)] +
                       [Arr("text%d" % k, XCHG, data=t, offset=(5 * k) % 16) for k, t in enumerate(texts, start=1)],
                       [Arr("y", WORD, n=16 * W, expect=raw(y)), Arr("r", WORD, n=16 * W, expect=raw(r)),
                        Arr("v", WORD, n=16 * W, expect=raw(v))] +
                       [Arr("bad%d" % k, VERDICT, verdict=-1) for k in range(1, n)], call)


# -- host-only generators --------------------------------------------------------------
def _g_batch(d, masked):
    n = 2
    sizes = [65, 1, 64]
    for faulted in (False, True):
        objs, lo = [], 0
        for o, W in enumerate(sizes):
            objs.append(d.odo_prefix(n, W, W - 1 if faulted and o == len(sizes) - 1 else None, lo=lo))
            lo += W
        ins, outs, verdicts = [], [], []
        for o, od in enumerate(objs):
            for a in odo_arrs(od):
                a.name = "o%d_%s" % (o, a.name)
                ins.append(a)
            W = sizes[o]
            if masked:
                sec = d.secrets[10 * o:10 * o + W]
                ins.append(Arr("o%d_secrets" % o, WORD, data=sec))
                exp, ff = d.F.mask_input(sec, od)
            else:
                exp, ff = d.F.recombine_verify(od)
            outs.append(Arr("o%d_out" % o, WORD, n=16 * W, expect=raw(exp)))
            verdicts.append(ff)
        outs.append(Arr("ff", VERDICT, verdict=verdicts))
        K = len(sizes)

        def call(L, h, p, fl, s, K=K):
            from amphora_amd import _lib
            arr = (_lib._AmphOdo * (K * n))()
            for o in range(K):
                for j in range(n):
                    arr[o * n + j] = _lib._AmphOdo(*[p["o%d_%s%d" % (o, f, j)] for f in FIELD], 16 * sizes[o])
            outp = vps([p["o%d_out" % o] for o in range(K)])
            if masked:
                return L.amph_mask_input_batch(h, arr, n, K, vps([p["o%d_secrets" % o] for o in range(K)]),
                                               (C.c_size_t * K)(*sizes), outp, i64(p["ff"]), 0)
            return L.amph_recombine_verify_batch(h, arr, n, K, outp, i64(p["ff"]), 0)
        yield Plan("%s_batch faulted=%s T=%d" % ("mask_input" if masked else "recombine_verify", faulted, sum(sizes)),
                   ins, outs, call,
                   (None, E_VERIFY if faulted else OK))


def g_recombine_verify_batch(d):
    return _g_batch(d, False)


def g_mask_input_batch(d):
    return _g_batch(d, True)


def g_party_host(d):
    """amph_party_begin / _text (out_cap exactly text_len, and text_len + 1) /
    _partner / _finish and _finish_b64, party 0 of n."""
    for n in (2, 3):
        for W in SESSION_SIZES:
            for b64 in (False, True):
                share, mk, tr, _ = d.pre(0, W)
                (y, r, v, mag, neg), ow, ou = _session_expect(d, n, W)
                own = jackson(FC.signed_of(mag, neg))
                texts = [d.pre_text(j, W) for j in range(1, n)]
                nc = 4 * ((16 * W + 2) // 3)
                outs = [Arr("y", WORD, n=16 * W, expect=raw(y)), Arr("r", WORD, n=16 * W, expect=raw(r)),
                        Arr("v", WORD, n=16 * W, expect=raw(v)),
                        Arr("own", XCHG, n=len(own), expect=own, offset=3),
                        Arr("own1", XCHG, n=len(own) + 1, expect=own, offset=7)]
                outs += [Arr("bad%d" % k, VERDICT, verdict=-1) for k in range(1, n)]
                if b64:
                    outs += [Arr("f%d" % k, B64, n=nc, expect=base64.b64encode(raw(x)), offset=k)
                             for k, x in enumerate((y, r, v, ow, ou))]
                else:
                    outs += [Arr("w", WORD, n=16 * W, expect=raw(ow)), Arr("u", WORD, n=16 * W, expect=raw(ou))]

                def call(L, h, p, fl, s, n=n, W=W, own=own, texts=texts, b64=b64):
                    ph = C.c_void_p()
                    st = L.amph_party_begin(h, p["share"], 32, p["masks"], p["triples"], W, n, p["y"], p["r"], p["v"],
                                            C.byref(ph))
                    if st:
                        return st
                    try:
                        assert L.amph_party_text_len(ph) == len(own) and L.amph_party_words(ph) == W
                        st = L.amph_party_text(ph, p["own"], len(own)) or L.amph_party_text(ph, p["own1"], len(own) + 1)
                        for k, t in enumerate(texts, start=1):
                            st = st or L.amph_party_partner(ph, k, p["text%d" % k], len(t), i64(p["bad%d" % k]))
                        if b64:
                            st = st or L.amph_party_finish_b64(ph, 1, vps([p["f%d" % k] for k in range(5)]))
                        else:
                            st = st or L.amph_party_finish(ph, 1, p["w"], p["u"])
                    finally:
                        L.amph_party_free(ph)
                    return st
                yield Plan("party_host n=%d W=%d b64=%s" % (n, W, b64),
                           [Arr("share", WORD, data=share), Arr("masks", WORD, data=mk), Arr("triples", WORD, data=tr)] +
                           [Arr("text%d" % k, XCHG, data=t, offset=(5 * k) % 16) for k, t in enumerate(texts, start=1)],
                           outs, call, (None, OK))


# ---- the table -----------------------------------------------------------------------
class Call:
    """names: the header symbols the entry drives; header: the lines of
    include/amphora.h that state its arrays' extents and alignment; modes:
    "device" (AMPH_F_DEVICE), "host"; lane: a one-word-per-lane kernel, also
    run under AMPH_BLOCK=64 / AMPH_GRID_CAP=3."""

    def __init__(self, names, header, modes, gen, lane=False):
        self.names = names if isinstance(names, tuple) else (names,)
        self.id, self.header, self.modes, self.gen, self.lane = gen.__name__[2:], header, modes, gen, lane


BOTH = ("device", "host")
CALLS = [
    Call("amph_recombine_verify", "43-50, 133-153, 242-248", BOTH, g_recombine_verify, lane=True),
    Call("amph_mask_input", "250-260", BOTH, g_mask_input, lane=True),
    Call("amph_recombine_verify_packed", "263-296", BOTH, g_recombine_verify_packed, lane=True),
    Call("amph_mask_input_packed", "263-299", BOTH, g_mask_input_packed, lane=True),
    Call("amph_recombine", "320-322", BOTH, g_recombine, lane=True),
    Call("amph_recombine_object", "323-328", BOTH, g_recombine_object, lane=True),
    Call("amph_verify", "330-335", BOTH, g_verify, lane=True),
    Call("amph_mask_words", "344-347", BOTH, g_mask_words, lane=True),
    Call("amph_to_gfp", "356-360", BOTH, g_to_gfp, lane=True),
    Call("amph_from_gfp", "356-362", BOTH, g_from_gfp, lane=True),
    Call("amph_convert_share", "365-373", BOTH, g_convert_share),
    Call("amph_odo_pre", "375-387", BOTH, g_odo_pre),
    Call("amph_open_diffs", "389-394", BOTH, g_open_diffs),
    Call("amph_odo_post", "396-400", BOTH, g_odo_post),
    Call("amph_open_post", "402-410", BOTH, g_open_post),
    Call("amph_base64_encode", "418, 428-429", BOTH, g_base64_encode),
    Call("amph_base64_decode", "419-431", BOTH, g_base64_decode),
    Call("amph_base64_encode_words", "427, 432-433", BOTH, g_base64_encode_words),
    Call("amph_base64_decode_words", "427, 434-435", BOTH, g_base64_decode_words),
    Call("amph_recombine_verify_b64", "449-469", BOTH, g_recombine_verify_b64),
    Call("amph_mask_input_b64", "470-482", BOTH, g_mask_input_b64),
    Call("amph_mask_input_b64", "472-482", BOTH, g_mask_input_b64_more_secrets),
    Call("amph_mask_input_json", "511-524", BOTH, g_mask_input_json),
    Call("amph_convert_share_json", "495-521", BOTH, g_convert_share_json),
    Call("amph_exchange_encode", "535-553", BOTH, g_exchange_encode),
    Call("amph_exchange_decode", "544-556", BOTH, g_exchange_decode),
    Call("amph_synth_odos", "650-657", ("device",), g_synth_odos, lane=True),
    Call("amph_synth_words", "658-659", ("device",), g_synth_words, lane=True),
    Call("amph_stream_probe", "660-667", ("device",), g_stream_probe, lane=True),
    Call(("amph_party_begin_dev", "amph_party_partner_dev", "amph_party_finish_b64_dev", "amph_party_text_dev"),
         "607-644", ("device",), g_party_dev),
    Call("amph_recombine_verify_batch", "301-315", ("host",), g_recombine_verify_batch),
    Call("amph_mask_input_batch", "301-318", ("host",), g_mask_input_batch),
    Call(("amph_party_begin", "amph_party_text", "amph_party_partner", "amph_party_finish", "amph_party_finish_b64"),
         "563-605", ("host",), g_party_host),
]

# Header symbols with no entry, and why.
LEFT_OUT = {
    "amph_verify_message": "host string rendering into (buf, cap); tests/test_abi.py pins the text",
    "amph_mask_word_host": "one word on the calling thread, no device work and no staging",
    "amph_ctx_create": "context call: no caller array", "amph_ctx_create_multi": "context call: no caller array",
    "amph_ctx_destroy": "context call: no caller array", "amph_ctx_device": "context call: no caller array",
    "amph_ctx_device_count": "context call: no caller array",
    "amph_ctx_set_batch_words": "context call: no caller array (used by the pipeline cases)",
    "amph_ctx_stats": "stats call: a fixed struct", "amph_host_register": "page-locks, writes nothing",
    "amph_host_unregister": "page-locks, writes nothing", "amph_time_next_launch": "timing call",
    "amph_timing_event_create": "timing call", "amph_timing_event_destroy": "timing call",
    "amph_timing_event_record": "timing call", "amph_timing_event_elapsed_ms": "timing call",
    "amph_strerror": "returns a string", "amph_last_error": "returns a string", "amph_version": "returns a string",
    "amph_build_id": "returns a string", "amph_exchange_max_chars": "pure function of a count",
    "amph_masked_input_data_chars": "pure function of a count",
    "amph_party_words": "reads a session field (asserted inside the party_host entry)",
    "amph_party_text_len": "reads a session field (asserted inside the party_host entry)",
    "amph_party_free": "frees a session (called by both session entries)",
    "amph_party_reset_partner": "frees a partner slot; writes no caller array",
}


def table_names():
    return sorted({n for c in CALLS for n in c.names})
