"""The text catalogue: honest base64 texts and named sets of byte edits to them,
with the text verdict (`bad_char`, `bad_chars`, `bad_index`) each one must get,
shared by tests/test_text_cases_cpu.py and tests/test_hip_texts.py; and MATRIX,
the calls the catalogue runs through (tests/test_text_cases_cpu.py holds it
against the headers).

The library decides "is this byte in the base64 alphabet" four times over: an
LDS table (b64.hpp dec_unit16_lut), a SWAR v_perm classifier (dec4_values6),
an exact locator (dec4_values) and a chain of compares (codec.hip dec6).  The
reference here is none of them: `first_bad` states the headers' rule in plain
Python, Python's base64 module says what an accepted text decodes to, and the
outputs follow from ``%`` on Python ints (tests/field_cases.py).

Four kinds of text (`first_bad(text, kind)`):

* field   one ODO field (amphora.h amph_odo_b64): the base64 of 16 W bytes;
          any byte outside A-Za-z0-9+/ before the final pad characters is
          refused, and anything but '=' inside them;
* record  24-character records: characters 0..21 in the alphabet, 22 and 23 '=';
* data    the MaskedInput "data" array text: '[', per record the 10 frame bytes
          {"value":" , the record, "} and ',' (']' after the last one);
* stream  amph_base64_decode: '=' only in the last one or two positions.

A case is a name, its class, byte edits ``(party, field, offset, byte)``, word
edits ``(party, field, index, new_word)`` made before the text is encoded, and
the verdict its construction DECLARES; `expect` recomputes the verdict with
`first_bad` and the outputs with Python's decode, and `self_check` asserts that
the two agree.  No expectation comes from the library under test.  An ordinary
module, not a conftest.
"""
from __future__ import annotations

import base64
import functools
from collections import namedtuple

from tests import field_cases as FC
from tests import verdict_cases as VC

ALPHABET = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/"
EQ = ord("=")
# the neighbours of each alphabet range ('+' '/' '0'-'9' 'A'-'Z' 'a'-'z') and the look-alikes
EDGE_BYTES = (0x00, 0x0A, 0x20, ord("*"), ord(","), ord("-"), ord("."), ord(":"), EQ, ord("@"), ord("["), ord("_"),
              ord("`"), ord("{"), 0x7F, 0x80, 0xAB, 0xAF, 0xB0, 0xC1, 0xE1, 0xFF)
SIZES = (1, 2, 3, 191, 192, 193, 194, 195)  # the paddings '==' '=' '' without and (from 193 on) with a fast tile
PARTIES = (1, 3, 5)                         # templated kernels (1, 3), the run-time party count (5)
RECORDS = 129                               # k_conv_json's 128-record tile and one more
PRIMES = ("test", "m89")                    # the test prime (BIG); !BIG for the ACCEPTED cases
TILE_CHARS, UNIT = 4096, 16                 # a wire workgroup's characters per field; one lane's unit
W_FULL = 193                                # one fast tile and a last tile of one whole unit and a padded one
FRAME_HEAD, FRAME_TAIL = b'{"value":"', b'"}'

# ---- the matrix ----------------------------------------------------------------------------
# Every declaration of include/*.h with a `bad_char`, `bad_chars` or `bad_index` parameter (a
# *_dev sibling through its base name) -> Entry(kind of text, the `form` parameter of the test
# of tests/test_hip_texts.py that runs the catalogue through it, what its header defines for a
# refused text besides the verdict).  tests/test_text_cases_cpu.py holds the table against the
# headers and the forms against the GPU file.
Entry = namedtuple("Entry", "kind form on_rejection")
_SINGLE = "host: AMPH_E_PARAM and the message; outputs and first_fail undefined"
_PACKED = "host: AMPH_E_PARAM, first_fail[o] = -1; the object's outputs undefined, every other object's written"
_SESSION = "the party's call and every finish report it; host mode writes no output; it outranks AMPH_E_VERIFY"
_SESSIONS = "per object, in the party's call and every finish; the other objects' outputs are written"
MATRIX = {
    "amph_base64_decode": Entry("stream", "stream", "host: AMPH_E_PARAM and the message; the output undefined"),
    "amph_base64_decode_words": Entry("record", "records",
                                      "the verdict is the RECORD's index (offset / 24); the output undefined"),
    "amph_recombine_verify_b64": Entry("field", "rv_b64", _SINGLE),
    "amph_mask_input_b64": Entry("field", "mask_b64", _SINGLE),
    "amph_mask_input_json": Entry("field", "mask_json", _SINGLE),
    "amph_convert_share_json": Entry("data", "convert_json", "host: AMPH_E_PARAM and the message; out_share undefined"),
    "amph_recombine_verify_b64_packed": Entry("field", "wire_packed", _PACKED),
    "amph_mask_input_b64_packed": Entry("field", "wire_packed", _PACKED),
    "amph_recombine_verify_b64_batch": Entry("field", "wire_batch", _PACKED),
    "amph_mask_input_b64_batch": Entry("field", "wire_batch", _PACKED),
    "amph_mask_input_json_packed": Entry("field", "upload_packed", _PACKED),
    "amph_mask_input_json_batch": Entry("field", "upload_batch", _PACKED),
    "amph_convert_share_json_packed": Entry("data", "convert_packed", "the object's own rows undefined"),
    "amph_convert_share_json_batch": Entry("data", "convert_batch", "the object's own rows undefined"),
    "amph_client_party": Entry("field", "client", _SESSION),
    "amph_client_finish_verify": Entry("field", "client", _SESSION),
    "amph_client_finish_mask": Entry("field", "client", _SESSION),
    "amph_client_finish_mask_json": Entry("field", "client", _SESSION),
    "amph_clients_party": Entry("field", "clients", _SESSIONS),
    "amph_clients_finish_verify": Entry("field", "clients", _SESSIONS),
    "amph_clients_finish_mask": Entry("field", "clients", _SESSIONS),
    "amph_clients_finish_mask_json": Entry("field", "clients", _SESSIONS),
}
_GRAMMAR = ("reads the Beaver exchange's JSON number grammar, not base64: a key of tests/exchange_cases.MATRIX, whose "
            "catalogue runs through it in tests/test_hip_exchange_texts.py")
LEFT_OUT = {name: _GRAMMAR for name in (
    "amph_exchange_decode", "amph_exchange_decode_packed", "amph_exchange_decode_batch",
    "amph_party_partner", "amph_parties_partner")}
# the forms that hold many objects per call: EDGE_BYTES x PLACES, PAIRS and ACCEPTED as objects
PACKED_FORMS = ("wire_packed", "upload_packed", "convert_packed", "clients")


# ---- the reference -----------------------------------------------------------------------
_OUTSIDE = bytes(0 if c in ALPHABET else 1 for c in range(256))


def byte_class(c: int) -> str:
    return "alphabet" if c in ALPHABET else "eq" if c == EQ else "high" if c >= 0x80 else "ascii"


@functools.lru_cache(maxsize=None)
def _only(c: int) -> bytes:
    """The translate table that marks every byte but `c`."""
    return bytes(0 if x == c else 1 for x in range(256))


def _outside(text: bytes) -> int:
    """The offset of the first byte outside the alphabet, or -1."""
    return text.translate(_OUTSIDE).find(1)


def field_pad(nchars: int) -> int:
    """The '=' count of the base64 of 16 W bytes in `nchars` characters."""
    assert nchars % 4 == 0
    fits = [pad for pad in (0, 1, 2) if (3 * nchars // 4 - pad) % 16 == 0]
    assert len(fits) == 1, nchars
    return fits[0]


def first_bad(text: bytes, kind: str) -> int:
    """The offset of the first byte the header's rule refuses, or -1."""
    n = len(text)
    if kind == "field":
        body = n - field_pad(n)
        at = _outside(text[:body])
        if at >= 0:
            return at
        return next((i for i in range(body, n) if text[i] != EQ), -1)
    if kind == "stream":
        assert n % 4 == 0 and n >= 4
        at = _outside(text[:n - 2])
        if at >= 0:
            return at
        for i in (n - 2, n - 1):
            legal_eq = text[i] == EQ and (i == n - 1 or text[n - 1] == EQ)
            if text[i] not in ALPHABET and not legal_eq:
                return i
        return -1
    # records: column q of every record at once (a strided slice), each against its own rule
    if kind == "record":
        assert n % 24 == 0
        rules = [_OUTSIDE] * 22 + [_only(EQ)] * 2
        hits = [24 * r + q for q in range(24) for r in [text[q::24].translate(rules[q]).find(1)] if r >= 0]
        return min(hits, default=-1)
    assert kind == "data"
    if text[:1] != b"[":
        return 0
    assert (n - 1) % 37 == 0 and n > 1
    body = text[1:]
    W = len(body) // 37
    record = FRAME_HEAD + bytes(24) + FRAME_TAIL + b","
    rules = [_OUTSIDE if 10 <= f < 32 else _only(EQ) if 32 <= f < 34 else _only(record[f]) for f in range(37)]
    hits = []
    for f in range(37):
        col = body[f::37]
        if f == 36:  # ',' after every record but the last, ']' after that one
            if col[-1:] != b"]":
                hits.append(37 * (W - 1) + f)
            col = col[:-1]
        r = col.translate(rules[f]).find(1)
        if r >= 0:
            hits.append(37 * r + f)
    return 1 + min(hits) if hits else -1


def decoded(text: bytes, kind: str) -> bytes:
    """The bytes an ACCEPTED text carries, by Python's base64 (which, as the
    headers say, ignores the unused low bits of the last data character)."""
    assert first_bad(text, kind) == -1
    if kind == "data":
        W = (len(text) - 1) // 37
        text = b"".join(text[1 + 37 * r + 10:1 + 37 * r + 34] for r in range(W))
        kind = "record"
    if kind == "record":
        return b"".join(base64.b64decode(text[r:r + 24], validate=True) for r in range(0, len(text), 24))
    return base64.b64decode(text, validate=True)


def words_of(raw: bytes) -> list:
    assert len(raw) % 16 == 0
    return [int.from_bytes(raw[i:i + 16], "little") for i in range(0, len(raw), 16)]


# ---- cases ------------------------------------------------------------------------------------
# edits: ((party, field, offset, byte), ...); word_edits: ((party, field, index, new_word), ...),
# made before the texts are encoded; want: the declared verdict (-1: accepted); place: a name of
# PLACES or None.  Single texts (record, data, stream) are party 0, field 0.
Case = namedtuple("Case", "name cls edits word_edits want place")
Expect = namedtuple("Expect", "bad ff changed")  # ff, changed ({word: new value}): None for a refused text


def wire_chars(W: int) -> int:
    return VC.wire_text_chars(W)


def code(nchars: int, party: int, field: int, offset: int) -> int:
    """bad_char of a wire-text call: (5 party + field) nchars + offset."""
    return (5 * party + field) * nchars + offset


def border_unit(nchars: int) -> int:
    """The last lane (unit) of a text with 16 (unit + 1) + 4 <= nchars: it decodes as the
    fast path does, the next unit character by character (wire.hip wire_fields, MIXED)."""
    return (nchars - 4) // UNIT - 1


def places(W: int) -> dict:
    """{name: offset} of a field text of W words.  The last two names of each pair straddle an
    edge: a dword, a unit, the fast / per-character lane border of the tile that holds the text's
    end, the tile itself.  `pad0` / `pad1` are the padding positions."""
    n = wire_chars(W)
    pad = field_pad(n)
    u = border_unit(n)
    out = {"first": 0, "dword_a": 3, "dword_b": 4, "unit_a": 15, "unit_b": 16, "mid": (n // 2) | 1,
           "border_a": UNIT * u + 15, "border_b": UNIT * (u + 1), "last_data": n - pad - 1}
    for i in range(pad):
        out["pad%d" % i] = n - pad + i
    if n > TILE_CHARS:
        out["tile_a"], out["tile_b"] = TILE_CHARS - 1, TILE_CHARS
    assert all(0 <= at < n for at in out.values()) and out["border_a"] >= 0
    return out


def place_bytes(name: str) -> tuple:
    """The bytes a place is tried with: every edge byte where data stands ('=' among them: '='
    in mid-text and at the last data character); where '=' must stand, every other edge byte
    and an alphabet character."""
    if name.startswith("pad"):
        return tuple(c for c in EDGE_BYTES if c != EQ) + (ord("A"),)
    return EDGE_BYTES


def place_classes(name: str) -> tuple:
    return ("ascii", "high", "alphabet") if name.startswith("pad") else ("ascii", "eq", "high")


def edge_cases(n: int, W: int) -> list:
    """EDGE_BYTES x PLACES(W): one offender per case, party and field rotating."""
    nc = wire_chars(W)
    out = []
    for name, at in places(W).items():
        for c in place_bytes(name):
            i = len(out)
            j, k = i % n, (i // n) % 5
            out.append(Case("edge_%s_%02x" % (name, c), "EDGE", ((j, k, at, c),), (), code(nc, j, k, at), name))
    return out


def diagonal(n: int, W: int) -> list:
    """Of edge_cases: each byte once, each (place, class) once, each place at least twice."""
    return _diagonal(edge_cases(n, W), list(places(W)), place_bytes, place_classes)


def _diagonal(all_cases, names, place_bytes, place_classes) -> list:
    by = {}
    for c in all_cases:
        by.setdefault((c.place, c.edits[0][3]), c)
    picked, seen = [], set()

    def take(place, byte):
        if (place, byte) in by and (place, byte) not in seen:
            seen.add((place, byte))
            picked.append(by[place, byte])

    for i, c in enumerate(EDGE_BYTES + (ord("A"),)):
        for d in range(len(names)):  # the next place (cyclically) that takes this byte
            name = names[(i + d) % len(names)]
            if c in place_bytes(name):
                take(name, c)
                break
    for name in names:
        for cls in place_classes(name):
            if not any(p == name and byte_class(b) == cls for p, b in seen):
                take(name, next(b for b in place_bytes(name) if byte_class(b) == cls))
        extra = iter(place_bytes(name))
        while sum(p == name for p, _ in seen) < 2:
            take(name, next(extra))
    return picked


def _base_word(b, j, k, i):
    return b.odos[j][k][i]


def pair_cases(b) -> list:
    """Several offenders in one call; and one together with a MAC fault."""
    n, W = b.n, b.W
    nc = wire_chars(W)
    j, k = n - 1, 2
    star, high, c1 = ord("*"), 0xFF, 0xC1
    out = [
        # one dword (characters 8..11): the non-ASCII byte first, and the reverse
        Case("pair_high_then_ascii", "PAIR", ((j, k, 8, high), (j, k, 9, star)), (), code(nc, j, k, 8), None),
        Case("pair_ascii_then_high", "PAIR", ((j, k, 8, star), (j, k, 9, high)), (), code(nc, j, k, 8), None),
        # 0xC1 is 'A' with bit 7 set: a decoder that drops the bit finds the '*' behind it, or nothing
        Case("pair_c1_then_ascii", "PAIR", ((j, k, 9, c1), (j, k, 10, star)), (), code(nc, j, k, 9), None),
        Case("pair_high_last_of_dword", "PAIR", ((j, k, 11, high), (j, k, 12, star)), (), code(nc, j, k, 11), None),
        # one unit, different dwords
        Case("pair_two_dwords", "PAIR", ((j, k, 13, ord("_")), (j, k, 2, ord("-"))), (), code(nc, j, k, 2), None),
    ]
    if nc > TILE_CHARS:  # one in each of two tiles, the later one listed first
        out.append(Case("pair_two_tiles", "PAIR", ((0, 4, TILE_CHARS + 4, ord(".")), (0, 4, 7, ord("@"))), (),
                        code(nc, 0, 4, 7), None))
    if n >= 3:  # party-major and field-major orders disagree: (5 * 1 + 4) < (5 * 2 + 1) but field 1 < field 4
        out.append(Case("pair_party_major", "PAIR", ((2, 1, 10, ord("!")), (1, 4, 20, ord("!"))), (),
                        code(nc, 1, 4, 20), None))
    if W >= 2:  # a bad character in word 0's text and a MAC fault in the last word: the text verdict outranks
        w = _base_word(b, 0, VC.Wf, W - 1)
        out.append(Case("pair_with_mac_fault", "PAIR", ((0, VC.R, 5, star),),
                        ((0, VC.Wf, W - 1, w + 1 if w < VC.TOP else w - 1),), code(nc, 0, VC.R, 5), None))
    return out


def accepted_cases(b) -> list:
    """Edits the rule accepts: a valid substitution that changes a word (the MAC verdict and the
    outputs are then those of the decoded words), and non-zero spare bits in the last data
    character (nothing changes)."""
    n, W = b.n, b.W
    nc = wire_chars(W)
    pad = field_pad(nc)
    texts = field_texts(b)
    j = n - 1
    at = (nc // 2) | 1
    old = texts[j][VC.Y][at]
    out = [Case("accepted_substitution", "ACCEPTED", ((j, VC.Y, at, ALPHABET[(ALPHABET.index(old) + 1) % 64]),), (),
                -1, None)]
    if pad:  # 16 W bytes end 2 (pad 1) or 4 (pad 2) bits short of the last data character's six
        last = nc - pad - 1
        old = texts[0][VC.U][last]
        v = ALPHABET.index(old)
        assert v & (3 if pad == 1 else 15) == 0
        out.append(Case("accepted_spare_bits", "ACCEPTED", ((0, VC.U, last, ALPHABET[v | (3 if pad == 1 else 9)]),),
                        (), -1, None))
    return out


@functools.lru_cache(maxsize=None)
def field_texts(b) -> tuple:
    """[party][field] -> Python's base64 of the base's words; every one is accepted."""
    out = tuple(tuple(VC.b64(FC.arr(f)) for f in o) for o in b.odos)
    assert all(first_bad(t, "field") == -1 and len(t) == wire_chars(b.W) for o in out for t in o)
    return out


def apply(b, case) -> dict:
    """{(party, field): the edited text} of the fields a case touches."""
    texts = field_texts(b)
    out = {}
    by_field = {}
    for j, k, i, new in case.word_edits:
        by_field.setdefault((j, k), []).append((i, new))
    for (j, k), edits in by_field.items():
        words = list(b.odos[j][k])
        for i, new in edits:
            assert 0 <= new <= VC.TOP and new != words[i]
            words[i] = new
        out[j, k] = bytearray(VC.b64(FC.arr(words)))
    for j, k, at, c in case.edits:
        t = out.setdefault((j, k), bytearray(texts[j][k]))
        assert t[at] != c or case.cls == "FULL", (case.name, "the edit changes nothing")
        t[at] = c
    return {jk: bytes(t) for jk, t in out.items()}


def expect(b, case) -> Expect:
    """The verdict by `first_bad` over the edited fields (the others are the honest base's);
    for an accepted text, FC.recombine_verify on the words Python decodes, at the words that
    differ from the base's."""
    pr = FC.BY_ID[b.pid]
    edited = apply(b, case)
    nc = wire_chars(b.W)
    bads = [code(nc, j, k, at) for (j, k), t in edited.items() for at in [first_bad(t, "field")] if at >= 0]
    if bads:
        return Expect(min(bads), None, None)
    new = {jk: words_of(decoded(t, "field")) for jk, t in edited.items()}
    touched = sorted({i for (j, k), ws in new.items() for i in range(b.W) if ws[i] != b.odos[j][k][i]})
    rows = [[[new[j, k][i] if (j, k) in new else b.odos[j][k][i] for i in touched] for k in range(5)]
            for j in range(b.n)]
    ys, ff = FC.recombine_verify(pr, rows) if touched else ([], -1)
    return Expect(-1, touched[ff] if ff >= 0 else -1, {i: y for i, y in zip(touched, ys) if y != b.cols[VC.Y][i]})


def by_party(b, case) -> list:
    """Per party the verdict of ITS five texts alone (what a session's party call reports)."""
    nc = wire_chars(b.W)
    out = [-1] * b.n
    for (j, k), t in sorted(apply(b, case).items()):
        at = first_bad(t, "field")
        if at >= 0 and out[j] < 0:
            out[j] = code(nc, j, k, at)
    return out


def self_check(b, case_list) -> dict:
    """Each case's recomputed verdict is the one its construction declares; -> {class: count}."""
    seen = {}
    for c in case_list:
        e = expect(b, c)
        assert e.bad == c.want, (b.pid, b.n, b.W, c.name, e.bad, c.want)
        if c.cls == "ACCEPTED":
            assert e.bad == -1
            assert (c.name == "accepted_substitution") == (e.ff >= 0 and bool(e.changed)), (c.name, e)
        seen[c.cls] = seen.get(c.cls, 0) + 1
    return seen


@functools.lru_cache(maxsize=None)
def catalogue(pid: str, n: int, W: int, which: str = "edge+pairs+accepted"):
    """(base, ((case, expect), ...)) -- built and self-checked once.  `which`: 'edge' is
    EDGE_BYTES x PLACES(W), 'diagonal' its diagonal."""
    b = VC.base(pid, n, W)
    cs = []
    for part in which.split("+"):
        cs += {"edge": lambda: edge_cases(n, W), "diagonal": lambda: diagonal(n, W), "pairs": lambda: pair_cases(b),
               "accepted": lambda: accepted_cases(b)}[part]()
    self_check(b, cs)
    return b, tuple((c, expect(b, c)) for c in cs)


# ---- the many-objects forms: object o carries case o ---------------------------------------------
Packed = namedtuple("Packed", "pid n objects sizes woff foff field_chars")
PackedObject = namedtuple("PackedObject", "name base case expect")
HONEST = Case("honest", "CLEAN", (), (), -1, None)


@functools.lru_cache(maxsize=None)
def packed_objects(pid: str, n: int, which: str = "edge+pairs+accepted") -> Packed:
    """Every case of catalogue(pid, n, W, which) for W in SIZES as the objects of one call, a
    clean object of the same size after every third case."""
    objects = []
    for W in SIZES:
        b, cs = catalogue(pid, n, W, which)
        for q, (c, e) in enumerate(cs):
            objects.append(PackedObject("%d/%s" % (W, c.name), b, c, e))
            if q % 3 == 2:
                objects.append(PackedObject("%d/clean%d" % (W, q), b, HONEST, Expect(-1, -1, {})))
    sizes = [o.base.W for o in objects]
    woff, foff = [0], [0]
    for W in sizes:
        woff.append(woff[-1] + W)
        foff.append(foff[-1] + VC.wire_slot_chars(W))
    assert sum(o.case is HONEST for o in objects) >= len(objects) // 5
    return Packed(pid, n, tuple(objects), tuple(sizes), tuple(woff), tuple(foff[:-1]), foff[-1])


# ---- single texts: records, "data" arrays, the stream ---------------------------------------------
@functools.lru_cache(maxsize=None)
def record_words(count: int = RECORDS, seed: str = "text_cases/records") -> tuple:
    import random
    rng = random.Random(seed)
    return tuple(rng.getrandbits(128) for _ in range(count))


def records_text(words) -> bytes:
    return b"".join(VC.record(w) for w in words)


def single_text(kind: str) -> bytes:
    """The honest text of a single-text kind: 129 records, their "data" array, or (stream) the
    base64 of 193 words: a whole 4,096-character block, one whole unit and a padded one."""
    if kind == "record":
        return records_text(record_words())
    if kind == "data":
        return VC.data_text(record_words())
    assert kind == "stream"
    return VC.b64(FC.arr(record_words(W_FULL, "text_cases/stream")))


def data_offset(record: int, q: int) -> int:
    """The offset of character q of a record in the "data" array text."""
    return 1 + 37 * record + 10 + q


EDGE_RECORDS = (0, 127, 128)  # the first record; the last of k_conv_json's first tile; the next, which is the last
RECORD_Q = (0, 3, 4, 15, 16, 21, 22, 23)  # dword and unit edges, the last data character, the two '='


def single_places(kind: str) -> dict:
    """{name: (offset, the bytes tried there, the classes among them, the declared verdict)}."""
    out = {}
    if kind == "stream":
        n = len(single_text("stream"))
        assert field_pad(n) == 2
        for name, at in places(W_FULL).items():
            if name.startswith("pad"):  # "=*": the '=' in front of a last character that is no '=' is refused
                out[name] = (at, tuple(c for c in EDGE_BYTES if c != EQ), ("ascii", "high"), n - 2)
            else:
                out[name] = (at, EDGE_BYTES, ("ascii", "eq", "high"), at)
        return out
    text = single_text(kind)
    for r in EDGE_RECORDS:
        for q in RECORD_Q:
            at = data_offset(r, q) if kind == "data" else 24 * r + q
            if q >= 22:
                out["r%d_q%d" % (r, q)] = (at, tuple(c for c in EDGE_BYTES if c != EQ) + (ord("A"),),
                                          ("ascii", "high", "alphabet"), at)
            else:
                out["r%d_q%d" % (r, q)] = (at, EDGE_BYTES, ("ascii", "eq", "high"), at)
        if kind == "data":  # frame bytes: '{', the '"' in front of the record, the '"' behind it, ',' / ']'
            for name, f in (("open", 0), ("quote", 9), ("close", 34), ("sep", 36)):
                at = 1 + 37 * r + f
                out["r%d_%s" % (r, name)] = (at, tuple(c for c in EDGE_BYTES if c != text[at]),
                                             ("ascii", "eq", "high"), at)
    if kind == "data":
        out["lead"] = (0, tuple(c for c in EDGE_BYTES if c != ord("[")), ("ascii", "eq", "high"), 0)
    return out


def single_edge_cases(kind: str) -> list:
    out = []
    for name, (at, tried, _, want) in single_places(kind).items():
        out += [Case("edge_%s_%02x" % (name, c), "EDGE", ((0, 0, at, c),), (), want, name) for c in tried]
    return out


def single_diagonal(kind: str) -> list:
    P = single_places(kind)
    return _diagonal(single_edge_cases(kind), list(P), lambda name: P[name][1], lambda name: P[name][2])


def single_pairs(kind: str) -> list:
    """Two offenders in one dword, the non-ASCII one first and the reverse; in one unit."""
    at = (lambda q: data_offset(5, q)) if kind == "data" else (lambda q: 24 * 5 + q) if kind == "record" else \
        (lambda q: UNIT * 5 + q)
    star, high, c1 = ord("*"), 0xFF, 0xC1
    return [Case("pair_high_then_ascii", "PAIR", ((0, 0, at(8), high), (0, 0, at(9), star)), (), at(8), None),
            Case("pair_ascii_then_high", "PAIR", ((0, 0, at(8), star), (0, 0, at(9), high)), (), at(8), None),
            Case("pair_c1_then_ascii", "PAIR", ((0, 0, at(9), c1), (0, 0, at(10), star)), (), at(9), None),
            Case("pair_two_dwords", "PAIR", ((0, 0, at(13), ord("_")), (0, 0, at(2), ord("-"))), (), at(2), None)]


def single_self_check(kind: str, case_list):
    text = single_text(kind)
    assert first_bad(text, kind) == -1
    for c in case_list:
        got = first_bad(edited_single(text, c), kind)
        assert got == c.want, (kind, c.name, got, c.want)


# ---- FULL and LATIN: one decoder implementation each -------------------------------------------------
# impl -> (kind of text, positions of its unit, where (value v, position q) of FULL goes: a unit
# or record index).  `wire_fast` and `wire_last` are the first and the last tile of a field text
# of 193 words (units 0..255 through the LDS table; unit 256 character by character through the
# SWAR classifier and the exact locator); `stream_block` is a whole block of amph_base64_decode
# (SWAR), `stream_tail` its last workgroup (dec6).
Impl = namedtuple("Impl", "kind positions unit")
IMPLS = {
    "wire_fast": Impl("field", 16, lambda v, q: (v + 37 * q) % 256),
    "wire_last": Impl("field", 16, lambda v, q: 256),
    "convert_json": Impl("data", 22, lambda v, q: (v + 5 * q) % RECORDS),
    "records": Impl("record", 22, lambda v, q: (3 * v + q) % RECORDS),
    "stream_block": Impl("stream", 16, lambda v, q: (5 * v + q) % 256),
    "stream_tail": Impl("stream", 16, lambda v, q: 256),
}
# which of the library's four deciders judges the cases of an impl (the summary's count)
DECIDERS = {"wire_fast": "LDS table (and the exact locator)", "wire_last": "SWAR classifier and exact locator",
            "convert_json": "SWAR classifier", "records": "SWAR classifier", "stream_block": "SWAR classifier",
            "stream_tail": "dec6"}


def impl_offset(impl: str, unit: int, q: int) -> int:
    kind = IMPLS[impl].kind
    return data_offset(unit, q) if kind == "data" else 24 * unit + q if kind == "record" else UNIT * unit + q


def full_cases(impl: str, n: int = 1) -> list:
    """256 byte values x the positions of a unit, one offender per case.  Declared: an alphabet
    character is accepted wherever it stands, every other byte is refused at its offset."""
    I = IMPLS[impl]
    nc = wire_chars(W_FULL)
    out = []
    for v in range(256):
        for q in range(I.positions):
            at = impl_offset(impl, I.unit(v, q), q)
            j, k = ((v + q) % n, (v // 3 + q) % 5) if I.kind == "field" else (0, 0)
            bad = -1 if v in ALPHABET else code(nc, j, k, at) if I.kind == "field" else at
            out.append(Case("full_%02x_%d" % (v, q), "FULL", ((j, k, at, v),), (), bad, None))
    return out


def latin_rows(impl: str) -> list:
    """[(unit, its characters)]: unit r, position q holds ALPHABET[(r + 5 q) % 64] -- every
    character at every position.  Where an impl has one unit only, 64 texts hold one row each."""
    I = IMPLS[impl]
    return [(I.unit(0, 0) if impl in ("wire_last", "stream_tail") else r,
             bytes(ALPHABET[(r + 5 * q) % 64] for q in range(I.positions))) for r in range(64)]


def latin_cases(impl: str, n: int) -> list:
    """LATIN on a field text as cases (class FULL: an edit may restate the character that is
    there): the last party's y field holds all 64 rows, or (`wire_last`) 64 cases hold one row
    each, in a field that rotates."""
    assert IMPLS[impl].kind == "field"
    j, rows = n - 1, latin_rows(impl)
    edits = lambda unit, row, k: tuple((j, k, impl_offset(impl, unit, q), row[q]) for q in range(len(row)))  # noqa: E731
    if impl == "wire_last":
        return [Case("latin_row%d" % r, "FULL", edits(unit, row, r % 5), (), -1, None)
                for r, (unit, row) in enumerate(rows)]
    return [Case("latin", "FULL", sum((edits(unit, row, VC.Y) for unit, row in rows), ()), (), -1, None)]


def latin_texts(impl: str, text: bytes) -> list:
    """The honest `text` with the LATIN rows written in: one text with all 64 rows, or 64 texts."""
    one_unit = impl in ("wire_last", "stream_tail")
    out, t = [], bytearray(text)
    for unit, row in latin_rows(impl):
        if one_unit:
            t = bytearray(text)
        at = impl_offset(impl, unit, 0)
        t[at:at + len(row)] = row
        if one_unit:
            out.append(bytes(t))
    return out if one_unit else [bytes(t)]


def edited_single(text: bytes, case) -> bytes:
    t = bytearray(text)
    for _, _, at, c in case.edits:
        t[at] = c
    return bytes(t)


def verdict_of(kind: str, bad: int) -> int:
    """The verdict a call reports for the reference's offset: amph_base64_decode_words names
    the record, every other call the byte."""
    return bad // 24 if kind == "record" and bad >= 0 else bad
