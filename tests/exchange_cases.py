"""The exchange-text catalogue: honest Beaver exchange texts
``[{"a":<d>,"b":<e>},...]`` and named edits to them, with the verdict
(`bad_index` and the status kind) and the values each one must get, shared by
tests/test_exchange_cases_cpu.py and tests/test_hip_exchange_texts.py; and
MATRIX, the calls the catalogue runs through (the CPU file holds it against
the headers).

The library reads this text with four parsers (exchange.hip: fast_segment,
fast_value, fast_number and the general grammar of xdec_general_span), built
from SWAR byte classes, dword masks and staged windows.  The reference here is
none of them, and has no span, window or word in it:

* `parse_pairs(text)` is a recursive-descent reader of the grammar
  include/amphora.h states for decode.  It decides accept or reject, and the
  values.
* `first_bad(text, npairs)` restates the header's offset rule: values are
  numbered by the colon before them, a value's token starts at the first
  non-blank byte after its colon, and the verdict is the smallest of the token
  starts of the values that are no NUM or whose surroundings break the grammar,
  and the offending byte of a missing bracket or of a non-blank byte in an
  array that must be empty; a text with no such defect and too few values
  gets `len` (AMPH_E_LEN).

A case is a name, its class, the text, the pair count the call expects and
the verdict its construction DECLARES; `expect` recomputes the verdict with
`first_bad` and the values with `parse_pairs`, and `self_check` asserts that
the two agree.  No expectation comes from the library under test.  An ordinary
module, not a conftest.
"""
from __future__ import annotations

import functools
import json
from collections import namedtuple

WS = b" \t\n\r"
DIGITS = b"0123456789"
TOP = 1 << 128
SPAN = 8192                 # the text one parse workgroup reads
WINDOW_TEXT = 16656         # a text at least this long: span 1's window lies wholly inside it
ENTRY = 92                  # one longest entry: {"a":-<39 digits>,"b":-<39 digits>},
MAX_STARTS = 1280           # the colons one span may hold
ALIGN = (0, 1, 15)          # the pointer offsets from a 16-byte boundary the single host call is tried at
COLON, MINUS, ZERO = 0x3A, 0x2D, 0x30
# the whitespace bytes and their control-byte neighbours, the neighbours of the digit and colon
# ranges, and every structural byte with bit 7 set
EDGE_BYTES = (0x00, 0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x1F, 0x20, ord("+"), ord("-"), ord("."), ord("/"), ord(":"),
              ord(";"), ord("e"), ord("E"), ord("\\"), ord("'"), 0x7F, 0x80, 0xA2, 0xAD, 0xB0, 0xB5, 0xB9, 0xBA,
              0xDB, 0xFB, 0xFD, 0xFF)

# ---- the matrix ----------------------------------------------------------------------------
# Every declaration of include/*.h that reads an exchange text (a *_dev sibling through its base
# name) -> Entry(the `form` parameter of tests/test_hip_exchange_texts.py that runs the catalogue
# through it, the modes it runs in, what its header defines for a refused text).
Entry = namedtuple("Entry", "form modes on_rejection")
MATRIX = {
    "amph_exchange_decode": Entry("single", ("host", "device"),
                                  "host: AMPH_E_PARAM / AMPH_E_LEN, *bad_index and the message; device: the "
                                  "verdict word; mag16 / neg undefined"),
    "amph_exchange_decode_packed": Entry("packed", ("host", "device"),
                                         "bad_index[o]; the object's own rows undefined, every other object's "
                                         "written"),
    "amph_exchange_decode_batch": Entry("batch", ("host",), "as the packed form's"),
    "amph_party_partner": Entry("party", ("host", "device"),
                                "the status, *bad_index and the message; host: the slot stays free; device: the "
                                "fields come out poisoned"),
    "amph_parties_partner": Entry("parties", ("host", "device"),
                                  "bad_index[o]; the object's fields begin \"!!!!\", every other object's are "
                                  "written"),
}


# ---- the reference -----------------------------------------------------------------------
def parse_pairs(text: bytes):
    """The (a, b) pairs of an accepted text as signed Python ints, or None:
        ws [ ws ( pair ( ws , ws pair )* )? ws ] ws EOF
        pair = { ws key ws : ws NUM ws , ws key ws : ws NUM ws }
    the two keys "a" and "b" in either order, ws the four JSON whitespace bytes,
    NUM = -?(0|[1-9][0-9]{0,38}) below 2^128 in magnitude ("-0" is 0)."""
    n = len(text)

    def ws(i):
        while i < n and text[i] in WS:
            i += 1
        return i

    def byte(i, c):
        if i < n and text[i] == c:
            return i + 1
        raise ValueError(i)

    def key(i):
        if text[i:i + 3] not in (b'"a"', b'"b"'):
            raise ValueError(i)
        return text[i + 1], i + 3

    def num(i):
        start = i
        if i < n and text[i] == MINUS:
            i += 1
        first = i
        while i < n and text[i] in DIGITS:
            i += 1
        if i == first or i - first > 39 or (text[first] == ZERO and i - first > 1):
            raise ValueError(start)
        v = int(text[first:i])
        if v >= TOP:
            raise ValueError(start)
        return (-v if first > start else v), i

    def member(i):
        k, i = key(ws(i))
        i = byte(ws(i), COLON)
        v, i = num(ws(i))
        return k, v, ws(i)

    def pair(i):
        i = byte(i, ord("{"))
        k0, v0, i = member(i)
        i = byte(i, ord(","))
        k1, v1, i = member(i)
        i = byte(i, ord("}"))
        if k0 == k1:
            raise ValueError(i)
        return ((v0, v1) if k0 == ord("a") else (v1, v0)), i

    try:
        out = []
        i = byte(ws(0), ord("["))
        i = ws(i)
        if i < n and text[i] == ord("{"):
            while True:
                p, i = pair(i)
                out.append(p)
                i = ws(i)
                if i < n and text[i] == ord(","):
                    i = ws(i + 1)
                    continue
                break
        i = ws(byte(i, ord("]")))
        if i != n:
            raise ValueError(i)
        return out
    except ValueError:
        return None


Verdict = namedtuple("Verdict", "kind bad")  # kind: "ok" (bad = -1), "param", "len" (bad = len(text))
# The planted errors of the decoder model (tests/test_exchange_cases_cpu.py): `scan` with one of
# these names is a decoder that is wrong in that one way.
FLAWS = ("control_bytes_are_whitespace", "bit7_dropped", "leading_zero", "forty_digits", "wraps_at_2_128",
         "plus_sign", "lone_minus_is_zero", "minus_zero_keeps_its_sign", "same_key_twice", "opener_not_tied",
         "bytes_after_the_bracket", "last_defect", "len_before_param", "offset_from_the_span",
         "offset_from_the_aligned_base", "offset_from_the_buffer")


def scan(text: bytes, npairs: int, flaw: str = None, mis: int = 0, slot: int = 0):
    """-> (Verdict, [(magnitude, sign byte), ...] by pair and key, or None).  With flaw=None the
    header's rule; `mis` and `slot` (the text's misalignment and its offset in a packed buffer)
    matter to a flawed decoder only."""
    assert flaw is None or flaw in FLAWS, flaw
    if flaw == "bit7_dropped":
        text = bytes(c & 0x7F for c in text)
    if flaw == "bytes_after_the_bracket" and b"]" in text:
        text = text[:text.index(b"]") + 1]
    blank = WS + b"\0\x0b\x0c" if flaw == "control_bytes_are_whitespace" else WS
    n, nvals = len(text), 2 * npairs

    def fwd(i):  # the first non-blank byte at or after i
        while i < n and text[i] in blank:
            i += 1
        return i

    def back(i):  # one past the last non-blank byte before i
        while i > 0 and text[i - 1] in blank:
            i -= 1
        return i

    def at(i, c):
        return 0 <= i < n and text[i] == c

    defects = []
    a, z = fwd(0), back(n)
    if not at(a, ord("[")):
        defects.append(a)
    elif z <= a + 1 or text[z - 1] != ord("]"):
        defects.append(z - 1)
    if nvals == 0:
        defects += [i for i in range(a + 1, z - 1) if text[i] not in blank][:1]
    values, colon, g = [], text.find(b":"), 0
    prev_end = prev_key = None
    while colon >= 0:
        x = fwd(colon + 1)                                   # the token start
        if defects and x > min(defects) and flaw != "last_defect":
            break
        ok = g < nvals
        p = back(colon)                                      # the key: "a" or "b"
        key = text[p - 2] if p >= 3 and text[p - 3:p] in (b'"a"', b'"b"') else 0
        ok = ok and key != 0
        q = back(p - 3) if key else 0
        if g % 2 == 0:                                       # the opener: '[' ws '{' / <digit> ws '}' ws ',' ws '{'
            ok = ok and at(q - 1, ord("{"))
            r = back(q - 1)
            if g == 0:
                ok = ok and at(r - 1, ord("[")) and back(r - 1) == 0
                tie = None
            else:
                ok = ok and at(r - 1, ord(","))
                r = back(r - 1)
                ok = ok and at(r - 1, ord("}"))
                tie = back(r - 1)
                ok = ok and tie > 0 and text[tie - 1] in DIGITS
        else:                                                # ',' between the members
            ok = ok and at(q - 1, ord(","))
            tie = back(q - 1)
        i = x                                                # the token: a NUM
        neg = at(i, MINUS) or (flaw == "plus_sign" and at(i, ord("+")))
        i += neg
        neg = neg and text[x] == MINUS
        first = i
        while i < n and text[i] in DIGITS and i - first < 41:
            i += 1
        nd = i - first
        end = i
        if flaw == "lone_minus_is_zero" and nd == 0 and neg:
            v = 0
        elif nd == 0 or nd > (40 if flaw == "forty_digits" else 39):
            ok, v = False, 0
        else:
            v = int(text[first:first + min(nd, 39)])
            if text[first] == ZERO and nd > 1 and flaw != "leading_zero":
                ok = False
            if v >= TOP:
                ok, v = ok and flaw == "wraps_at_2_128", v % TOP
        j = fwd(end)                                         # what closes the member
        ok = ok and at(j, ord(",") if g % 2 == 0 else ord("}"))
        if g + 1 == nvals:                                   # the last value closes the array: '}' ws ']' ws EOF
            j = fwd(j + 1)
            ok = ok and at(j, ord("]")) and fwd(j + 1) == n
        if g > 0 and ok:                                     # tied to the value before it
            if flaw != "opener_not_tied":
                ok = tie == prev_end
            if g % 2 == 1 and flaw != "same_key_twice":
                ok = ok and key != prev_key
        if not ok:
            defects.append(x)
        values.append((key, v, 1 if neg and (v or flaw == "minus_zero_keeps_its_sign") else 0))
        prev_end, prev_key = end, key
        colon, g = text.find(b":", colon + 1), g + 1
    count = text.count(b":")
    if flaw == "len_before_param" and count != nvals:
        defects = []
    if defects:
        bad = max(defects) if flaw == "last_defect" else min(defects)
    elif count != nvals:
        bad = n
    else:
        out = []
        for k in range(0, nvals, 2):
            (k0, v0, s0), (k1, v1, s1) = values[k], values[k + 1]
            out += [(v0, s0), (v1, s1)] if k0 == ord("a") else [(v1, s1), (v0, s0)]
        return Verdict("ok", -1), out
    kind = "len" if bad == n else "param"
    if flaw == "offset_from_the_span":
        bad %= SPAN
    if flaw == "offset_from_the_aligned_base":
        bad += mis
    if flaw == "offset_from_the_buffer":
        bad += slot
    return Verdict(kind, bad), None


def first_bad(text: bytes, npairs: int) -> Verdict:
    """The header's verdict for `text` where `npairs` pairs are expected."""
    return scan(text, npairs)[0]


def diffs_of(pairs) -> list:
    """[(magnitude, sign byte)] in the calls' order (a then b) of parse_pairs' pairs."""
    return [(abs(v), 1 if v < 0 else 0) for p in pairs for v in p]


# ---- texts ---------------------------------------------------------------------------------
def compact(pairs) -> bytes:
    """Jackson's compact output (tests/test_wire.py establishes the identity)."""
    return json.dumps([{"a": a, "b": b} for a, b in pairs], separators=(",", ":")).encode()


def number(nd: int, seed: int) -> int:
    """A positive number of exactly nd digits below 2^128."""
    if nd == 1:
        return seed % 9 + 1
    v = 10 ** (nd - 1) + (seed * 7919 + 12345) % (10 ** (nd - 1))
    return v if v < TOP else 10 ** 38 + seed


def long_pairs(count: int, seed: int, nd: int = 30) -> list:
    out = []
    for k in range(count):
        a, b = number(nd + (seed + k) % 5, seed + 2 * k), number(nd + (seed + 3 * k) % 5, seed + 2 * k + 1)
        out.append((-a if (seed + k) % 5 == 0 else a, -b if (seed + k) % 7 == 0 else b))
    return out


def slot_chars(npairs: int) -> int:
    return -(-(ENTRY * npairs + 2) // SPAN) * SPAN


TEMPLATE = (-12, 345)
SEGMENT = b'},{"a":-12,"b":345},{"'   # behind the digit before it: positions 0 .. 22
Placed = namedtuple("Placed", "text npairs D P")  # D: offset of the digit before the template pair's '},'; P: that value's token


@functools.lru_cache(maxsize=None)
def placed(D: int, min_len: int = 0) -> Placed:
    """A compact text whose TEMPLATE pair stands with the digit before its '},' at offset D, by
    the choice of the digit counts before it; at least min_len characters, an even pair count
    that a session slot of that many pairs holds."""
    count = max(1, (D + 1) // 80)
    before = long_pairs(count, D)
    grow = D + 1 - (len(compact(before)) - 2)
    assert 0 <= grow <= 8 * count, (D, grow)
    out = []
    for a, b in before:  # lengthen the numbers a digit at a time (no number passes 38 digits)
        vals = []
        for v in (a, b):
            add = min(4, grow)
            grow -= add
            vals.append((abs(v) * 10 ** add + add) * (-1 if v < 0 else 1))
        out.append(tuple(vals))
    before = out
    after = long_pairs(2, D + 1)
    while True:
        text = compact(before + [TEMPLATE] + after)
        if len(text) >= min_len and (len(before) + 1 + len(after)) % 2 == 0:
            break
        after += long_pairs(1, D + len(after))
    npairs = len(before) + 1 + len(after)
    assert text[D + 1:D + 1 + len(SEGMENT)] == SEGMENT and text[D] in DIGITS and len(text) <= slot_chars(npairs)
    assert parse_pairs(text) == before + [TEMPLATE] + after
    return Placed(text, npairs, D, text.rindex(b":", 0, D) + 1)


def declare(where: str, j: int, c: int, D: int, P: int, n: int) -> Verdict:
    """What byte c at position j of the template's segment must get, from the grammar's words.
    Positions: 0 the digit before, then SEGMENT: 1 '}' 2 ',' 3 '{' 4 '"' 5 'a' 6 '"' 7 ':' 8 '-'
    9 '1' 10 '2' 11 ',' 12 '"' 13 'b' 14 '"' 15 ':' 16 '3' 17 '4' 18 '5' 19 '}' 20 ',' 21 '{'
    22 '"'.  where: "interior"; "first" (D = -2: position 2 is the text's '['); "last" (position
    20 is the text's ']').  A, B, N: the token starts of the template's values and of the next one."""
    A, B, N = D + 8, D + 16, D + 26
    blank, digit = c in WS, c in DIGITS
    was = ord("[") if (where, j) == ("first", 2) else ord("]") if (where, j) == ("last", 20) else SEGMENT[j - 1] if j \
        else None
    if c == was:                          # the byte that stands there
        return Verdict("ok", -1)
    if where == "first" and j == 2:       # '[': a blank moves the complaint to the '{' behind it
        return Verdict("param", 1 if blank else 0)
    if where == "last" and j == 20:       # ']': the last value does not close the array
        return Verdict("param", B)
    accepted = {0: blank or digit,                       # the value before: one digit shorter, or another digit
                8: blank or (digit and c != ZERO),       # ' 12', '712'; '012' has a leading zero
                9: digit and c != ZERO,                  # '-02' has one
                10: blank or digit,                      # '-1 ,' and '-17,'
                16: blank or c == MINUS or (digit and c != ZERO),
                17: digit,
                18: blank or digit}.get(j, False)
    if accepted:
        return Verdict("ok", -1)
    if where == "last" and j == 15:       # the last value's colon gone: nothing is malformed, one value is missing
        return Verdict("len", n)
    # whose surroundings the byte belongs to: the value before (its '}'), the template's a (its
    # opener, key, token and ','), its b (key, token and '}'), the next value (its opener).  A
    # colon gone renumbers what follows: the next value is then the wrong member.
    anchor = P if j < 2 else B if j == 7 else A if j < 12 else N if j == 15 else B if j < 20 else N
    if j == 5 and c == ord("b"):          # the same key twice: reported at the second
        anchor = B
    if j == 0 and c == ord("}"):          # '206}},{': the value before is closed, a's opener finds no digit behind '}'
        anchor = A
    if j == 10 and c == ord(","):         # '-1,,"b"': a ends at its ',', b's ',' does not follow a's last digit
        anchor = B
    if j in (17, 18) and c == ord("}") and where != "last":  # '3}5},{': b is closed, the next opener is not tied to it
        anchor = N
    if c == COLON:                        # a new colon numbers a value of its own: its token is the next byte
        anchor = min(anchor, D + j + 1)
    return Verdict("param", anchor)


# ---- cases ------------------------------------------------------------------------------------
# place: a name of PLACES or None; role: (digit count, member role) for NUMBERS or None
Case = namedtuple("Case", "name cls text npairs want place role")
# pairs: parse_pairs' pairs, None for a refused text; parsed: what parse_pairs made of the text, whatever the count
Expect = namedtuple("Expect", "kind bad pairs parsed")
CLASSES = ("FULL", "EDGE", "NUMBERS", "PAIRS", "ACCEPTED")
ROLES = ("member0", "member1", "first", "last")
SWEEPS = {"first": range(2, 23), "interior": range(0, 23), "last": range(0, 21)}  # the positions FULL tries


def poke(text: bytes, at: int, c) -> bytes:
    c = bytes([c]) if isinstance(c, int) else c
    return text[:at] + c + text[at + len(c):]


def _case(name, cls, text, npairs, want, place=None, role=None):
    return Case(name, cls, text, npairs, Verdict(*want), place, role)


FULL_PAIRS = {"first": [TEMPLATE, (70, -81), (9, 10)], "interior": [(7, 2065), TEMPLATE, (-9, 10)],
              "last": [(1, -2), (70, 2065), TEMPLATE]}


def sweep_geometry(where: str):
    """(text, D, P) of FULL's three-pair text for a sweep."""
    text = compact(FULL_PAIRS[where])
    D = -2 if where == "first" else text.rindex(SEGMENT[:-3]) - 1
    P = text.rindex(b":", 0, D) + 1 if D > 0 else None
    return text, D, P


@functools.lru_cache(maxsize=None)
def full_cases() -> tuple:
    """All 256 byte values at every position of a value's segment: the first pair (with '[{'),
    an interior one, the last (with '}]' and the end); three pairs a text."""
    out = []
    for where, positions in SWEEPS.items():
        text, D, P = sweep_geometry(where)
        for j in positions:
            for c in range(256):
                out.append(_case("full_%s_%02d_%02x" % (where, j, c), "FULL", poke(text, D + j, c), 3,
                                 declare(where, j, c, D, P, len(text)), where))
    return tuple(out)


BORDER_D = tuple(range(SPAN - 1 - 22, SPAN + 1))   # D for which some segment position stands at 8191 or 8192
INTERIOR_D = 12001                                  # span 1, far from both its borders
BLANKS = 257                                        # one more than the window pad
SMALL = compact([TEMPLATE, (70, -2065), (-9, 10), TEMPLATE])


def edge_places() -> dict:
    """{place: [(where, text, npairs, D, P, j), ...]}: the spots EDGE_BYTES are tried at."""
    out = {"border_8191": [], "border_8192": [], "span1": [], "first6": [], "last2": []}
    for D in BORDER_D:
        pl = placed(D, SPAN + 200)
        for T in (SPAN - 1, SPAN):
            if 0 <= T - D <= 22:
                out["border_%d" % T].append(("interior", pl.text, pl.npairs, D, pl.P, T - D))
    pl = placed(INTERIOR_D, WINDOW_TEXT + 64)
    assert SPAN + 256 < INTERIOR_D < 2 * SPAN - 256 - 23 and len(pl.text) >= WINDOW_TEXT
    out["span1"] = [("interior", pl.text, pl.npairs, INTERIOR_D, pl.P, j) for j in range(23)]
    out["first6"] = [("first", SMALL, 4, -2, None, j) for j in range(2, 8)]
    D = SMALL.rindex(SEGMENT[:-3]) - 1
    out["last2"] = [("last", SMALL, 4, D, SMALL.rindex(b":", 0, D) + 1, j) for j in (19, 20)]
    return out


PLACES = ("border_8191", "border_8192", "span1", "first6", "last2", "blanks257")


@functools.lru_cache(maxsize=None)
def edge_cases() -> tuple:
    """EDGE_BYTES x PLACES."""
    out = []
    for place, spots in edge_places().items():
        for where, text, npairs, D, P, j in spots:
            for c in EDGE_BYTES:
                if text[D + j] != c:
                    out.append(_case("edge_%s_D%d_%02d_%02x" % (place, D, j, c), "EDGE", poke(text, D + j, c), npairs,
                                     declare(where, j, c, D, P, len(text)), place))
    # the first value behind 257 blanks: the token's first byte
    text = b'[{"a":' + b" " * BLANKS + compact([TEMPLATE, (70, 81)])[6:]
    at = 6 + BLANKS
    assert text[at] == MINUS and parse_pairs(text) == [TEMPLATE, (70, 81)]
    for c in EDGE_BYTES:
        if c != MINUS:
            out.append(_case("edge_blanks257_%02x" % c, "EDGE", poke(text, at, c), 2,
                             ("ok", -1) if c in WS else ("param", at), "blanks257"))
    return tuple(out)


def role_text(token: bytes, role: str):
    """(a four-pair compact text with `token` as a value in `role`, the token's offset)."""
    objs = [b'{"a":-7,"b":21}', b'{"a":65,"b":-2}', b'{"a":3,"b":40}', b'{"a":-5,"b":6}']
    k, m = {"member0": (1, b"a"), "member1": (2, b"b"), "first": (0, b"a"), "last": (3, b"b")}[role]
    head = b'{"a":' if m == b"a" else objs[k][:objs[k].index(b'"b":') + 4]
    tail = objs[k][objs[k].index(b","):] if m == b"a" else b"}"
    objs[k] = head + token + tail
    text = b"[" + b",".join(objs) + b"]"
    return text, len(b"[" + b",".join(objs[:k]) + (b"," if k else b"")) + len(head)


BAD_TOKENS = (b"-", b"--1", b"-00", b"01", b"1.5", b"1e5", b'"1"', b"%d" % TOP, b"-%d" % TOP, b"%d" % 10 ** 39,
              b"-%d" % 10 ** 39, b"1234567890" * 4, b"-" + b"9" * 40)


@functools.lru_cache(maxsize=None)
def number_cases() -> tuple:
    out = []
    for role in ROLES:
        for nd in range(1, 40):
            lo, hi = (10 ** (nd - 1) if nd > 1 else 0), min(10 ** nd - 1, TOP - 1)
            for which, v in (("least", lo), ("greatest", hi), ("minus_least", -lo), ("minus_greatest", -hi)):
                text, _ = role_text(b"%d" % v, role)
                out.append(_case("number_%s_%d_%s" % (role, nd, which), "NUMBERS", text, 4, ("ok", -1), None, (nd, role)))
        text, at = role_text(b"-0", role)
        out.append(_case("number_%s_minus_zero" % role, "NUMBERS", text, 4, ("ok", -1), None, (1, role)))
        for tok in BAD_TOKENS:
            text, at = role_text(tok, role)
            out.append(_case("number_%s_bad_%s" % (role, tok[:12].decode()), "NUMBERS", text, 4, ("param", at)))
    # a 39-digit negative number with each of its 40 characters at the span border in turn
    tok = b"-%d" % (TOP - 1)
    for k in range(40):
        pl = placed(SPAN - 8 - k, SPAN + 200)   # the template's a token stands at 8192 - k
        A = pl.D + 8
        text = pl.text[:A] + tok + pl.text[A + 3:]
        assert text[SPAN - k:SPAN - k + 40] == tok and len(text) <= slot_chars(pl.npairs)
        out.append(_case("number_border_%02d" % k, "NUMBERS", text, pl.npairs, ("ok", -1), "border_8192", (39, "member0")))
    # 2^128 in span 1 of a text whose window lies inside it
    pl = placed(INTERIOR_D, WINDOW_TEXT + 64)
    text = pl.text[:pl.D + 8] + b"%d" % TOP + pl.text[pl.D + 11:]
    assert len(text) <= slot_chars(pl.npairs)
    out.append(_case("number_2_128_in_span1", "NUMBERS", text, pl.npairs, ("param", pl.D + 8), "span1"))
    return tuple(out)


DENSE = compact([(k % 9 + 1, (k + 4) % 9 + 1) for k in range(640)])   # 1,280 values, 1,170 of them in span 0


@functools.lru_cache(maxsize=None)
def pair_cases() -> tuple:
    """PAIRS and STRUCTURE: each text by hand, its verdict from where its parts stand."""
    four = [(1, 2), (-30, 4), (5, -60), (7, 8)]
    T = compact(four)
    mid = T.index(b'{"a":-30')           # the second pair's '{'
    A1, B1 = mid + 5, T.index(b'"b":4') + 4
    A2 = T.index(b'"a":5') + 4
    out = [
        _case("same_key_twice", "PAIRS", T.replace(b'"b":4', b'"a":4'), 4, ("param", B1)),
        _case("third_member", "PAIRS", T.replace(b'"b":4}', b'"b":4,"a":3}'), 4, ("param", B1)),
        _case("stray_value_between_members", "PAIRS", T.replace(b'-30,', b'-30,7,'), 4, ("param", B1 + 2)),
        _case("stray_bytes_after_a_pair", "PAIRS", T.replace(b'"b":4}', b'"b":4}5}'), 4, ("param", A2 + 2)),
        _case("two_commas", "PAIRS", T.replace(b'4},{', b'4},,{'), 4, ("param", A2 + 1)),
        _case("missing_open_bracket", "PAIRS", T[1:], 4, ("param", 0)),
        _case("doubled_open_bracket", "PAIRS", b"[" + T, 4, ("param", 7)),
        _case("missing_close_bracket", "PAIRS", T[:-1], 4, ("param", T.rindex(b":") + 1)),
        _case("doubled_close_bracket", "PAIRS", T + b"]", 4, ("param", T.rindex(b":") + 1)),
        _case("bytes_after_the_array", "PAIRS", T + b" [", 4, ("param", T.rindex(b":") + 1)),
        _case("blank_then_bytes_after_the_array", "PAIRS", T + b"\n\n0", 4, ("param", T.rindex(b":") + 1)),
        _case("empty_one_pair_expected", "PAIRS", b"[]", 1, ("len", 2)),
        _case("empty_two_pairs_expected", "PAIRS", b"[]", 2, ("len", 2)),
        _case("one_pair_none_expected", "PAIRS", b'[{"a":1,"b":2}]', 0, ("param", 1)),
        _case("two_pairs_too_few", "PAIRS", compact(four[:2]), 4, ("len", len(compact(four[:2])))),
        # too few pairs and bytes behind the last of them: the header settles it as the count's verdict
        _case("two_pairs_too_few_then_stray_bytes", "PAIRS", compact(four[:2])[:-1] + b"x]", 4,
              ("len", len(compact(four[:2])) + 1)),
        _case("two_pairs_too_many", "PAIRS", compact(four + four[:2]), 4,
              ("param", T.rindex(b":") + 1)),                       # the fourth pair must close the array
        _case("two_defects", "PAIRS", poke(poke(T, A2, b"x"), A1, b"+"), 4, ("param", A1)),
        _case("two_defects_later_first_in_the_text", "PAIRS", poke(poke(T, A1, b"+"), A2, b"x"), 4, ("param", A1)),
        # a defect in a text whose count is wrong too: the malformed token, never the count
        _case("defect_and_too_few", "PAIRS", poke(compact(four[:2]), A1, b"x"), 4, ("param", A1)),
        _case("defect_and_too_many", "PAIRS", poke(compact(four + four), A1, b"x"), 4, ("param", A1)),
        _case("key_with_a_backslash", "PAIRS", T.replace(b'"a":5', b'"\\u0061":5'), 4, ("param", A2 + 5)),
    ]
    # across a span border: the stray-bytes tie, and two defects either side of it
    pl = placed(SPAN - 7, SPAN + 200)
    A = pl.D + 8
    stray = pl.text[:pl.D + 1] + b"}5" + pl.text[pl.D + 1:]
    assert pl.P < SPAN <= A + 2 - 1 and len(stray) <= slot_chars(pl.npairs)
    out.append(_case("stray_bytes_tie_across_the_border", "PAIRS", stray, pl.npairs, ("param", A + 2), "border_8192"))
    pl = placed(SPAN - 12, SPAN + 200)
    A, B = pl.D + 8, pl.D + 16
    assert A < SPAN <= B
    out.append(_case("two_defects_either_side_of_the_border", "PAIRS", poke(poke(pl.text, B, b";"), A, b"/"),
                     pl.npairs, ("param", A), "border_8192"))
    out.append(_case("defect_behind_the_border_only", "PAIRS", poke(pl.text, B, b";"), pl.npairs, ("param", B),
                     "border_8192"))
    # one case with its defect in span 1 of a text whose window lies inside it
    pl = placed(INTERIOR_D, WINDOW_TEXT + 64)
    out.append(_case("same_key_twice_in_span1", "PAIRS", poke(pl.text, pl.D + 13, b"a"), pl.npairs,
                     ("param", pl.D + 16), "span1"))
    # more colons than a span may hold: a legal dense stretch just under it, and a flood
    assert DENSE[:SPAN].count(b":") < MAX_STARTS < DENSE.count(b":") + 1 and len(DENSE) > SPAN
    out.append(_case("dense_colons_legal", "ACCEPTED", DENSE, 640, ("ok", -1)))
    cut = DENSE.index(b":", 1400) + 1
    flood = DENSE[:cut] + b":" * (MAX_STARTS + 20) + DENSE[cut:]
    assert flood[:SPAN].count(b":") > MAX_STARTS
    out.append(_case("colon_flood", "PAIRS", flood, 640, ("param", cut), "flood"))
    return tuple(out)


GAPS = (b'{ "a":-12,"b":345}', b'{"a" :-12,"b":345}', b'{"a": -12,"b":345}', b'{"a":-12 ,"b":345}',
        b'{"a":-12, "b":345}', b'{"a":-12,"b" :345}', b'{"a":-12,"b": 345}', b'{"a":-12,"b":345 }')


@functools.lru_cache(maxsize=None)
def accepted_cases() -> tuple:
    pairs = long_pairs(6, 3, 10) + [(0, -1), TEMPLATE]
    items = [{"a": a, "b": b} for a, b in pairs]
    swapped = [{"b": b, "a": a} if k % 2 == 0 else {"a": a, "b": b} for k, (a, b) in enumerate(pairs)]
    out = [
        _case("pretty_printed", "ACCEPTED", json.dumps(items, indent=2).encode(), 8, ("ok", -1)),
        _case("b_before_a", "ACCEPTED", json.dumps(swapped, separators=(",", ":")).encode(), 8, ("ok", -1)),
        _case("keys_swapped_in_one_pair", "ACCEPTED", compact(pairs).replace(b'{"a":-12,"b":345}', b'{"b":-12,"a":345}'),
              8, ("ok", -1)),
    ]
    tokens = [b"["]
    for k, (a, b) in enumerate(pairs):
        tokens += [b"{", b'"a"', b":", b"%d" % a, b",", b'"b"', b":", b"%d" % b, b"}", b"," if k < 7 else b"]"]
    for name, blank in (("tabs", b"\t"), ("cr_lf", b"\r\n"), ("mixed", b" \t\r\n")):
        out.append(_case("blank_%s_between_every_two_tokens" % name, "ACCEPTED", blank + blank.join(tokens) + blank, 8,
                         ("ok", -1)))
    for run in (255, 256, 257):
        t = compact(pairs)
        out.append(_case("run_%d_before_a_value" % run, "ACCEPTED", t.replace(b'"b":345', b'"b":' + b" " * run + b"345"),
                         8, ("ok", -1)))
        out.append(_case("run_%d_before_the_bracket" % run, "ACCEPTED", t[:-1] + b"\n" * run + b"]", 8, ("ok", -1)))
    for k, obj in enumerate(GAPS):  # one blank at each gap of an interior pair, among compact pairs
        t = compact(pairs[:3] + [TEMPLATE] + pairs[3:7])
        assert t.count(b'{"a":-12,"b":345}') == 1
        out.append(_case("gap_%d" % k, "ACCEPTED", t.replace(b'{"a":-12,"b":345}', obj), 8, ("ok", -1)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def expect(case) -> Expect:
    """The verdict by `first_bad`, the values by `parse_pairs`."""
    v = first_bad(case.text, case.npairs)
    pairs = parse_pairs(case.text)
    return Expect(v.kind, v.bad, pairs if v.kind == "ok" else None, pairs)


def self_check(case_list) -> dict:
    """Each case's recomputed verdict is the one its construction declares, and the two
    references agree with each other; -> {class: count}."""
    seen = {}
    for c in case_list:
        e = expect(c)
        v, pairs = Verdict(e.kind, e.bad), e.parsed
        assert v == c.want, (c.name, v, c.want)
        if pairs is None:  # parse_pairs knows no count: what it refuses is refused whatever count is expected
            assert v.kind != "ok" and first_bad(c.text, c.text.count(b":") // 2).kind != "ok", (c.name, v)
        else:              # and what it accepts has no fault but, possibly, the count
            v2, values2 = scan(c.text, len(pairs))
            assert v2.kind == "ok" and values2 == diffs_of(pairs), (c.name, v2)
            assert (v.kind == "ok") == (len(pairs) == c.npairs), (c.name, v, len(pairs))
        assert v.kind != "len" or v.bad == len(c.text), c.name
        if c.place == "flood":   # at or before the first flooded colon: no span's capacity is in the rule
            assert v.kind == "param" and v.bad <= c.text.index(b"::") + 1, c.name
        if c.cls == "ACCEPTED":
            assert v.kind == "ok", c.name
        seen[c.cls] = seen.get(c.cls, 0) + 1
    return seen


BUILDERS = {"FULL": full_cases, "EDGE": edge_cases, "NUMBERS": number_cases, "PAIRS": pair_cases,
            "ACCEPTED": accepted_cases}


@functools.lru_cache(maxsize=None)
def catalogue(which: str = "FULL+EDGE+NUMBERS+PAIRS+ACCEPTED") -> tuple:
    """((case, expect), ...) of the classes named -- built and self-checked once."""
    cs = [c for part in which.split("+") for c in BUILDERS[part]()]
    assert len({c.name for c in cs}) == len(cs)
    self_check(cs)
    return tuple((c, expect(c)) for c in cs)


def diagonal() -> tuple:
    """One case of every class, one of every place, and every NUMBERS digit count (the roles in
    turn): what runs through the calls that take one text each."""
    picked, seen = [], set()
    for c, e in catalogue():
        keys = {("cls", c.cls, e.kind), ("place", c.place)} if c.place else {("cls", c.cls, e.kind)}
        if c.role and e.kind == "ok" and ROLES[c.role[0] % 4] == c.role[1]:
            keys.add(("digits", c.role[0]))
        if c.cls in ("PAIRS", "ACCEPTED") and c.npairs <= 8:
            keys.add(("name", c.name))
        if not keys <= seen:
            seen |= keys
            picked.append((c, e))
    return tuple(picked)


# ---- the many-objects forms: object o carries case o -----------------------------------------
CLEAN = compact(long_pairs(6, 11, 17))
Object = namedtuple("Object", "name text npairs expect clean")


def fits_a_session(c) -> bool:
    """A session's object is a whole number of words (two pairs each) and its text fits the slot
    its word count gives it."""
    return c.npairs % 2 == 0 and len(c.text) <= slot_chars(c.npairs)


@functools.lru_cache(maxsize=None)
def objects(which: str, session: bool = False) -> tuple:
    """The cases of catalogue(which) as the objects of one call, a clean compact object after
    every third; session: only what a session's object can be."""
    out = []
    clean = Expect("ok", -1, parse_pairs(CLEAN), parse_pairs(CLEAN))
    for c, e in catalogue(which):
        if session and not fits_a_session(c):
            continue
        out.append(Object(c.name, c.text, c.npairs, e, False))
        if len(out) % 4 == 3:
            out.append(Object("clean%d" % len(out), CLEAN, 6, clean, True))
    assert sum(o.clean for o in out) >= len(out) // 5
    return tuple(out)
