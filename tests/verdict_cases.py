"""The verdict catalogue: honest ODO rows and named sets of edits to them, with
the verdict each one must get, shared by tests/test_verdict_cpu.py and
tests/test_hip_verdicts.py; and MATRIX, the calls the catalogue runs through
(tests/test_session_cases_cpu.py holds it against the headers).

Every verifying call ends in ``ok = (y r == w) & (v r == u)``.  The catalogue
holds, for one prime, party count and word count,

* A  one field (y, r, v, w, u), one word, one party's share off: reject there;
* B  a change that is no fault mod p (+ p, + k p, +1 / -1 on two parties): accept;
* C  both equalities hold for the wrong pair (w' = v r with u' = y r; y and v
     exchanged): reject;
* D  a changed field with its MACs changed to match: accept, from the words read;
* E  several faults in different fields: the smallest index wins.

A case is a name, its class, a list of ``(party, field, index, new_word)``
edits and the verdict its construction DECLARES (`want_ff`, `y_changes`).
`expect` computes the verdict with ``%`` on Python ints
(tests/field_cases.py recombine_verify); `self_check` asserts the two agree,
so a base whose values do not make a case decisive fails on the CPU.  No
expectation comes from the library under test.  An ordinary module, not a
conftest.
"""
from __future__ import annotations

import base64
import functools
import random
from collections import namedtuple

import numpy as np

from tests import field_cases as FC

FIELDS = ("y", "r", "v", "w", "u")  # ODO order
Y, R, V, Wf, U = range(5)
TOP = FC.M128 - 1
# with + 1 (limb 0) one bit in each 32-bit limb of the compare, and the top bit
LIMB_DELTAS = (("d32", 1 << 32), ("d64", 1 << 64), ("d96", 1 << 96), ("top", 1 << 127))

# The verdict matrix: every ABI call that takes a `first_fail` (a *_dev sibling
# through its base name) -> the `call` parameter of
# tests/test_hip_verdicts.py::test_verdicts that runs the catalogue through it.
# tests/test_session_cases_cpu.py holds this table against include/*.h.
MATRIX = {
    "amph_recombine_verify": "recombine_verify",
    "amph_mask_input": "mask_input",
    "amph_verify": "verify",
    "amph_recombine_verify_b64": "recombine_verify_b64",
    "amph_mask_input_b64": "mask_input_b64",
    "amph_mask_input_json": "mask_input_json",
    "amph_client_finish_verify": "client_verify",
    "amph_client_finish_mask": "client_mask",
    "amph_client_finish_mask_json": "client_mask_json",
    "amph_clients_finish_verify": "clients_verify",
    "amph_clients_finish_mask": "clients_mask",
    "amph_clients_finish_mask_json": "clients_mask_json",
    "amph_recombine_verify_packed": "packed",
    "amph_mask_input_packed": "packed",
    "amph_recombine_verify_batch": "batch",
    "amph_mask_input_batch": "batch",
    "amph_recombine_verify_b64_packed": "wire_packed",
    "amph_mask_input_b64_packed": "wire_packed",
    "amph_recombine_verify_b64_batch": "wire_batch",
    "amph_mask_input_b64_batch": "wire_batch",
    "amph_mask_input_json_packed": "upload_packed",
    "amph_mask_input_json_batch": "upload_batch",
}
MATRIX_LEFT_OUT = {}  # {ABI symbol with a first_fail: why the matrix does not run it}

Base = namedtuple("Base", "pid n W odos cols")         # odos[party][field][i] raw words, cols[field][i] canonical
Case = namedtuple("Case", "name cls edits want_ff y_changes limb")
Expect = namedtuple("Expect", "ff changed")             # changed: {index: new canonical secret}


# ---- base rows -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def base(pid: str, n: int, W: int, seed: int = 0x7E2D1C7) -> Base:
    """Honest ODOs of n parties over W words.  Parties 0..n-2 hold uniform raw
    128-bit words in all five fields (words >= p occur); the last party closes
    every sum, canonical on even words and + k p on odd ones (FC.lift).  The
    recombined y, r, v are nonzero and pairwise distinct at EVERY word, so a
    fault in any one field breaks exactly the equalities it stands in."""
    pr = FC.BY_ID[pid]
    rng = random.Random("%d/%s/%d/%d" % (seed, pid, n, W))
    cols = [[0] * W for _ in range(5)]
    odos = [[[0] * W for _ in range(5)] for _ in range(n)]
    for i in range(W):
        while True:
            y, r, v = (rng.randrange(1, pr.p) for _ in range(3))
            if len({y, r, v}) == 3:
                break
        vals = (y, r, v, y * r % pr.p, v * r % pr.p)
        for k in range(5):
            cols[k][i] = vals[k]
            rest = FC.to_gfp(pr, vals[k])
            for j in range(n - 1):
                odos[j][k][i] = rng.getrandbits(128)
                rest = (rest - odos[j][k][i]) % pr.p
            odos[n - 1][k][i] = FC.lift(pr, rest, i)
    b = Base(pid, n, W, tuple(tuple(tuple(f) for f in o) for o in odos), tuple(tuple(c) for c in cols))
    # on the inputs: decisive at every word, honest by the plain reference, words >= p present
    for i in range(W):
        assert 0 not in (b.cols[Y][i], b.cols[R][i], b.cols[V][i])
        assert len({b.cols[Y][i], b.cols[R][i], b.cols[V][i]}) == 3
    assert FC.recombine_verify(pr, b.odos) == (list(b.cols[Y]), -1)
    if W >= 64:
        for k in range(5):
            assert any(w >= pr.p for o in b.odos for w in o[k]), (pid, n, k)
    return b


def secrets_for(b: Base) -> list:
    """Raw secret words for the masking calls (>= p included, fixed seed)."""
    rng = random.Random("secrets/%s/%d/%d" % (b.pid, b.n, b.W))
    return [rng.getrandbits(128) for _ in range(b.W)]


# ---- building cases ----------------------------------------------------------------
def _find(W: int, start: int, ok):
    """The first word from `start` on (cyclically) that fits, or None."""
    for d in range(W):
        i = (start + d) % W
        if ok(i):
            return i
    return None


def _pick(W: int, start: int, ok) -> int:
    i = _find(W, start, ok)
    assert i is not None, "no word of the base fits the case"
    return i


def _close(b: Base, k: int, i: int, value: int):
    """The last party's share word that makes field k recombine to `value`
    at word i, in Montgomery form via to_gfp -- one edit."""
    pr = FC.BY_ID[b.pid]
    rest = FC.to_gfp(pr, value % pr.p)
    for j in range(b.n - 1):
        rest = (rest - b.odos[j][k][i]) % pr.p
    return (b.n - 1, k, i, rest)


def off_by_one(b: Base, j: int, k: int, i: int):
    """Party j's share of field k at word i off by one, without wrapping."""
    w = b.odos[j][k][i]
    return (j, k, i, w + 1 if w < TOP else w - 1)


def single_fault(b: Base, field: int, i: int, party: int = 0, name: str | None = None) -> Case:
    return Case(name or "A_%s_at%d" % (FIELDS[field], i), "A", (off_by_one(b, party, field, i),), i,
                frozenset({i}) if field == Y else frozenset(), None)


def _parties(n: int):
    return (0, n // 2, n - 1)  # first, middle, last


def cases(b: Base, classes: str = "ABCDE") -> list:
    pr = FC.BY_ID[b.pid]
    n, W, p = b.n, b.W, pr.p
    rot = _parties(n)
    word = lambda j, k, i: b.odos[j][k][i]  # noqa: E731
    out = []
    none = frozenset()

    if "A" in classes:
        mont = lambda k, i: FC.to_gfp(pr, b.cols[k][i])  # noqa: E731  (the canonical Montgomery sum a kernel compares)

        def one_bit(j, k, d, start):
            """(word, limb): a word where party j's share + d fits and turns exactly
            bit d of the compared sum; where the prime (or a tiny base) has none,
            a plain fault of that size."""
            i = _find(W, start, lambda i: word(j, k, i) + d <= TOP and not mont(k, i) & d and mont(k, i) + d < p)
            if i is not None:
                return i, word(j, k, i) + d, (d.bit_length() - 1) // 32
            i = _pick(W, start, lambda i: word(j, k, i) + d <= TOP or word(j, k, i) >= d)
            return i, (word(j, k, i) + d if word(j, k, i) + d <= TOP else word(j, k, i) - d), None

        starts = (0, W - 1, W // 2, 64, 63)
        for k in range(5):
            j = rot[k % 3]
            if k in (Wf, U):
                i, new, limb = one_bit(j, k, 1, starts[k] % W)
            else:
                i = _pick(W, starts[k] % W, lambda i: word(j, k, i) < TOP)
                new, limb = word(j, k, i) + 1, None
            out.append(Case("A_%s_plus1" % FIELDS[k], "A", ((j, k, i, new),), i, frozenset({i}) if k == Y else none, limb))
        for k in (Wf, U):
            for q, (tag, d) in enumerate(LIMB_DELTAS):
                i, new, limb = one_bit(rot[(q + k) % 3], k, d, (97 * (q + 1) + 31 * k) % W)
                out.append(Case("A_%s_%s" % (FIELDS[k], tag), "A", ((rot[(q + k) % 3], k, i, new),), i, none, limb))

    if "B" in classes:
        for k in range(5):
            j = rot[(k + 1) % 3]
            i = _pick(W, (5 + 50 * k) % W, lambda i: word(j, k, i) + p <= TOP)
            out.append(Case("B_%s_plus_p" % FIELDS[k], "B", ((j, k, i, word(j, k, i) + p),), -1, none, None))
            if b.pid == "m89":
                j = rot[(k + 2) % 3]
                i = _pick(W, (9 + 40 * k) % W, lambda i: (TOP - word(j, k, i)) // p >= 2)
                kk = (TOP - word(j, k, i)) // p
                out.append(Case("B_%s_plus_kp" % FIELDS[k], "B", ((j, k, i, word(j, k, i) + kk * p),), -1, none, None))
        if n >= 2:
            for k in (Wf, U):
                i = _pick(W, (33 + 7 * k) % W, lambda i: 0 < word(0, k, i) < TOP and 0 < word(n - 1, k, i) < TOP)
                out.append(Case("B_%s_cancel" % FIELDS[k], "B",
                                ((0, k, i, word(0, k, i) + 1), (n - 1, k, i, word(n - 1, k, i) - 1)), -1, none, None))

    c = b.cols
    if "C" in classes:
        i = 70 % W
        out.append(Case("C_wu_crossed", "C", (_close(b, Wf, i, c[V][i] * c[R][i]), _close(b, U, i, c[Y][i] * c[R][i])),
                        i, none, None))
        i = 129 % W
        out.append(Case("C_yv_exchanged", "C", (_close(b, Y, i, c[V][i]), _close(b, V, i, c[Y][i])), i,
                        frozenset({i}), None))

    if "D" in classes:
        i = 65 % W
        out.append(Case("D_y_with_w", "D", (_close(b, Y, i, c[Y][i] + 1), _close(b, Wf, i, c[Wf][i] + c[R][i])), -1,
                        frozenset({i}), None))
        i = 127 % W
        out.append(Case("D_v_with_u", "D", (_close(b, V, i, c[V][i] + 1), _close(b, U, i, c[U][i] + c[R][i])), -1,
                        none, None))
        i = 200 % W
        out.append(Case("D_r_with_w_u", "D", (_close(b, R, i, c[R][i] + 1), _close(b, Wf, i, c[Wf][i] + c[Y][i]),
                                             _close(b, U, i, c[U][i] + c[V][i])), -1, none, None))

    if "E" in classes:
        sets = [("E_63w_64u", {63: Wf, 64: U}), ("E_64w_63u", {64: Wf, 63: U}), ("E_191u_192w", {191: U, 192: Wf}),
                ("E_1023v_1024u", {1023: V, 1024: U}), ("E_0u_lastv", {0: U, W - 1: V})]
        for name, faults in sets:
            if max(faults) >= W or len(faults) < 2 or (name == "E_0u_lastv" and W < 2):
                continue
            edits = tuple(off_by_one(b, rot[(q + i) % 3], k, i) for q, (i, k) in enumerate(sorted(faults.items())))
            out.append(Case(name, "E", edits, min(faults), none, None))
        out.append(Case("E_u_everywhere", "E", tuple(off_by_one(b, rot[i % 3], U, i) for i in range(W)), 0, none, None))
        out.append(Case("E_u_last", "E", (off_by_one(b, n - 1, U, W - 1),), W - 1, none, None))
    return out


# ---- the reference -------------------------------------------------------------------
def edited_rows(b: Base, case: Case, touched):
    """The parties' five fields at the touched words only, edits applied."""
    at = {i: q for q, i in enumerate(touched)}
    rows = [[[f[i] for i in touched] for f in o] for o in b.odos]
    for j, k, i, new in case.edits:
        assert 0 <= new <= TOP and new != b.odos[j][k][i], case.name
        rows[j][k][at[i]] = new
    return rows


def expect(b: Base, case: Case) -> Expect:
    """FC.recombine_verify on the edited rows.  Untouched words are the honest
    base's (verified by the same function in `base`), so only the touched ones
    are recomputed."""
    pr = FC.BY_ID[b.pid]
    touched = sorted({e[2] for e in case.edits})
    ys, ff = FC.recombine_verify(pr, edited_rows(b, case, touched))
    return Expect(touched[ff] if ff >= 0 else -1,
                  {i: y for i, y in zip(touched, ys) if y != b.cols[Y][i]})


def columns(b: Base, case: Case):
    """The five recombined columns (canonical values) of the edited rows, for
    the calls that take them recombined: [y, r, v, w, u] lists."""
    pr = FC.BY_ID[b.pid]
    touched = sorted({e[2] for e in case.edits})
    rows = edited_rows(b, case, touched)
    cols = [list(col) for col in b.cols]
    for k in range(5):
        for i, x in zip(touched, FC.recombine(pr, [o[k] for o in rows])):
            cols[k][i] = x
    return cols


def self_check(b: Base, case_list) -> dict:
    """Each case's reference verdict is the one its construction declares;
    returns {class: count}."""
    pr = FC.BY_ID[b.pid]
    seen = {}
    for case in case_list:
        e = expect(b, case)
        assert e.ff == case.want_ff, (b.pid, b.n, case.name, e.ff, case.want_ff)
        assert set(e.changed) == set(case.y_changes), (b.pid, b.n, case.name)
        assert (case.cls in "ACE") == (e.ff >= 0), case.name
        if case.cls == "D":
            assert (case.name == "D_y_with_w") == bool(e.changed), case.name
        if case.limb is not None:  # exactly one limb of the compared Montgomery word differs
            (_, k, i, _), = case.edits
            old = FC.to_gfp(pr, b.cols[k][i])
            new = FC.to_gfp(pr, columns(b, case)[k][i])
            assert [(old ^ new) >> 32 * q & 0xFFFFFFFF != 0 for q in range(4)] == [q == case.limb for q in range(4)]
        seen[case.cls] = seen.get(case.cls, 0) + 1
    return seen


@functools.lru_cache(maxsize=None)
def catalogue(pid: str, n: int, W: int, classes: str = "ABCDE"):
    """(base, [(case, expect)]) -- built and self-checked once."""
    b = base(pid, n, W)
    cs = cases(b, classes)
    self_check(b, cs)
    return b, tuple((c, expect(b, c)) for c in cs)


# ---- arrays and texts ---------------------------------------------------------------
def base_arrays(b: Base):
    """Per party the five (W, 16) arrays, read-only (apply() copies what it edits)."""
    out = [[FC.arr(f) for f in o] for o in b.odos]
    for o in out:
        for f in o:
            f.setflags(write=False)
    return out


def apply(arrays, case: Case):
    """(arrays with the case's edits, the set of (party, field) that differ):
    edited fields are fresh copies, the others the base's own arrays."""
    out = [list(o) for o in arrays]
    hit = set()
    for j, k, i, new in case.edits:
        if (j, k) not in hit:
            out[j][k] = out[j][k].copy()
            hit.add((j, k))
        out[j][k][i] = np.frombuffer(int(new).to_bytes(16, "little"), np.uint8)
    return out, hit


def b64(a) -> bytes:
    """Python's base64 of a word array: the wire text of one field."""
    return base64.b64encode(np.ascontiguousarray(a).tobytes())


def patched(values, changed: dict) -> list:
    out = list(values)
    for i, x in changed.items():
        out[i] = x
    return out


# ---- the catalogue as objects of ONE client session (include/amphora_client_batch.h) -----------
# The K-secret session accumulates with one workgroup per 192-word tile of ONE object (k_acc_b64's
# segmented form, k_mask_sums_seg) and verifies with the word-packed k_rv_seg, where an object's
# border may lie inside a wave.  The layout below makes the tile prefix sums uneven, puts empty
# objects directly before and after failing ones and no failing object at word 0.
TILE = 192          # wiretiles.hpp kWireTileWords
WAVE = 64
W_SESSION = 257     # one object per catalogue case: two tiles, the second of 65 words
FILLER_SIZES = (0, 1, 192, 0, 193, 2, 385, 3, 191)

SessionObject = namedtuple("SessionObject", "name kind base case ff cols y secrets masked records text")
Session = namedtuple("Session", "pid n objects sizes woff foff uoff field_chars upload_chars ff")


def wire_text_chars(W: int) -> int:
    return 4 * ((16 * W + 2) // 3)


def wire_slot_chars(W: int) -> int:
    return (wire_text_chars(W) + 15) & ~15


def upload_text_chars(W: int) -> int:
    return 37 * W + 1 if W else 2


def upload_slot_chars(W: int) -> int:
    return (upload_text_chars(W) + 15) & ~15


def record(word: int) -> bytes:
    """Python's base64 of one 16-byte little-endian word: a 24-character record."""
    return base64.b64encode(int(word).to_bytes(16, "little"))


def data_text(words) -> bytes:
    """Jackson's compact MaskedInput "data" array of the given words ("[]" for none)."""
    return b"[" + b",".join(b'{"value":"' + record(w) + b'"}' for w in words) + b"]"


def tile_of(woff, o: int, i: int) -> int:
    """The workgroup that owns word i of object o: g(o) + i / 192 with g(o) = woff[o] / 192 + o."""
    return woff[o] // TILE + o + i // TILE


@functools.lru_cache(maxsize=None)
def _mask_refs(pid: str, n: int, W: int, y: tuple):
    """(secrets, masked words, records, framed text) of base(pid, n, W)'s secrets under the masks `y`."""
    secrets = tuple(secrets_for(base(pid, n, W)))
    masked = tuple(FC.mask_words(FC.BY_ID[pid], secrets, y))
    return secrets, masked, b"".join(record(m) for m in masked), data_text(masked)


def _session_object(b: Base, name: str, kind: str, case, e: Expect) -> SessionObject:
    """One object with every expected result, from Python ints alone (objects
    that recombine to the same secrets share one computation of the mask step)."""
    cols = tuple(tuple(c) for c in columns(b, case)) if case is not None and case.edits else b.cols
    y = tuple(patched(b.cols[Y], e.changed))
    assert y == tuple(cols[Y]), name  # two ways to the same secrets: `expect` and `columns`
    return SessionObject(name, kind, b, case, e.ff, cols, y, *_mask_refs(b.pid, b.n, b.W, y))


@functools.lru_cache(maxsize=None)
def session_objects(pid: str, n: int) -> Session:
    """The catalogue as the objects of one K-secret client session: an honest
    257-word object, one 257-word object per case of catalogue(pid, n, 257),
    then the pair (`u` off in the last word of one object, `w` off in word 0 of
    the next: the two objects stay neighbours).  After each of these -- the
    pair counting as one -- comes ONE honest filler whose size walks
    FILLER_SIZES, rows from `base` at that size.  Every object carries its
    expected verdict, secrets, masked words, records and framed text, computed
    with ``%`` on Python ints; the coverage predicates below are asserted on
    this layout alone, before any library call."""
    pr = FC.BY_ID[pid]
    b, cs = catalogue(pid, n, W_SESSION)
    W = b.W
    honest = Expect(-1, {})
    pair = [single_fault(b, U, W - 1, party=n - 1, name="pair_last_u"), single_fault(b, Wf, 0, party=0, name="pair_first_w")]
    units = [[_session_object(b, "honest", "honest", None, honest)]]
    units += [[_session_object(b, c.name, "case", c, e)] for c, e in cs]
    units.append([_session_object(b, c.name, "pair", c, expect(b, c)) for c in pair])
    objects = []
    for q, unit in enumerate(units):
        objects += unit
        fb = base(pid, n, FILLER_SIZES[q % len(FILLER_SIZES)])
        objects.append(_session_object(fb, "filler%d_%d" % (q, fb.W), "filler", None, honest))
    sizes = [o.base.W for o in objects]
    K = len(objects)

    def offsets(per):
        out = [0]
        for x in per:
            out.append(out[-1] + x)
        return out

    woff = offsets(sizes)
    foff = offsets([wire_slot_chars(w) for w in sizes])
    uoff = offsets([upload_slot_chars(w) for w in sizes])
    ff = [o.ff for o in objects]
    names = [o.name for o in objects]
    failing = [o for o in range(K) if ff[o] >= 0]
    # ---- the coverage predicates, on the inputs alone -------------------------------------
    assert len(names) == len(set(names)) and {c.cls for c, _ in cs} == set("ABCDE")
    assert all(o.ff == -1 for o in objects if o.kind in ("honest", "filler"))
    # no failing object starts at word 0: its local verdict differs from its packed index
    assert failing and all(woff[o] > 0 for o in failing)
    # a verdict in an object's second tile, and two faults that straddle the tile edge inside one object
    assert any(ff[o] >= TILE for o in failing)
    edge = objects[names.index("E_191u_192w")]
    assert {e[2] for e in edge.case.edits} == {TILE - 1, TILE} and edge.ff == TILE - 1 and edge.base.W > TILE
    # the pair: neighbours inside one 64-lane wave of the packed words (k_rv_seg) ...
    lo, hi = names.index("pair_last_u"), names.index("pair_first_w")
    g = woff[lo + 1] - 1
    assert hi == lo + 1 and woff[hi] == g + 1 and g // WAVE == (g + 1) // WAVE and (ff[lo], ff[hi]) == (W - 1, 0)
    # ... and in different objects' tiles (k_acc_b64, k_mask_sums_seg)
    assert tile_of(woff, lo, W - 1) != tile_of(woff, hi, 0)
    # an empty object directly before one failing object and directly after another
    assert any(sizes[o] == 0 and ff[o + 1] >= 0 for o in range(K - 1))
    assert any(sizes[o] == 0 and ff[o - 1] >= 0 for o in range(1, K))
    # a failing object at a packed offset that is no multiple of the tile
    assert any(woff[o] % TILE for o in failing)
    # every tile count and prefix the fillers are there for: uneven prefix sums
    assert len({woff[o] % TILE for o in range(K)}) > len(FILLER_SIZES)
    # words >= p in each of the five fields, from the first party and from the last
    for j in (0, n - 1):
        for k in range(5):
            assert any(w >= pr.p for w in b.odos[j][k]), (pid, n, j, k)
    return Session(pid, n, tuple(objects), tuple(sizes), tuple(woff), tuple(foff[:-1]), tuple(uoff[:-1]), foff[-1],
                   uoff[-1], tuple(ff))


def object_rows(obj: SessionObject):
    """[party][field] -> the object's raw words as ints, its case's edits applied."""
    rows = [list(o) for o in obj.base.odos]
    for j, k, i, new in (obj.case.edits if obj.case is not None else ()):
        if isinstance(rows[j][k], tuple):
            rows[j][k] = list(rows[j][k])
        rows[j][k][i] = new
    return rows


@functools.lru_cache(maxsize=None)
def _base_arrays_and_texts(pid: str, n: int, W: int):
    arrays = base_arrays(base(pid, n, W))
    return arrays, tuple(tuple(b64(f) for f in o) for o in arrays)


def object_texts(obj: SessionObject):
    """[party][field] -> Python's base64 of the object's words, edits applied
    (only the edited fields are encoded again)."""
    arrays, texts = _base_arrays_and_texts(obj.base.pid, obj.base.n, obj.base.W)
    out = [list(o) for o in texts]
    if obj.case is not None and obj.case.edits:
        edited, hit = apply(arrays, obj.case)
        for j, k in hit:
            out[j][k] = b64(edited[j][k])
    return out
