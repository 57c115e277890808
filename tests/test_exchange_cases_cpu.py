"""The exchange-text catalogue (tests/exchange_cases.py) cannot rot -- all on the CPU.

* Every declaration of include/*.h that reads an exchange text -- one with a
  `bad_index` that is no call of the base64 matrix (tests/text_cases.py) -- is
  a key of EC.MATRIX; the guard fails by the missing name; no key is stale;
  every form is a parameter of tests/test_hip_exchange_texts.py; the keys are
  those text_cases.LEFT_OUT hands over.
* `self_check` passes for every case: the verdict each case's construction
  declares is the one `first_bad` computes, and `parse_pairs` agrees with it.
* `parse_pairs` equals Python's json module (arranged to be as strict as the
  header) on every catalogue text, and `first_bad` reproduces every offset
  tests/test_wire.py pins.
* A single-byte substitution in a compact text is reported within one longest
  entry of the edit.
* The coverage the catalogue claims is there.
* A Python model of a decoder with ONE planted error each disagrees with the
  catalogue on at least one case: the cases are decisive.
"""
import json
import os
import re

import pytest

from tests import exchange_cases as EC
from tests import text_cases as TC
from tests.test_session_cases_cpu import declarations_with

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THE_FIVE = ("amph_exchange_decode", "amph_exchange_decode_packed", "amph_exchange_decode_batch",
            "amph_party_partner", "amph_parties_partner")


# ---- the matrix covers the headers ------------------------------------------------------------
def exchange_readers():
    """{name: header} of the declarations with a `bad_index` that the base64 matrix does not run."""
    def base(name):
        return name[:-4] if name.endswith("_dev") else name
    return {name: h for name, h in declarations_with("bad_index").items() if base(name) not in TC.MATRIX}


def check_exchange_matrix(found, matrix):
    for name, header in found.items():
        base = name[:-4] if name.endswith("_dev") else name
        assert base in matrix, "%s (%s) reads an exchange text and is in no exchange-text test" % (name, header)
    for name in matrix:  # no stale key
        assert name in found, "%s is not a declaration that reads an exchange text" % name
    for name in found:  # the _dev siblings run through their base names: the base is declared too
        if name.endswith("_dev"):
            assert name[:-4] in found, name


def test_the_matrix_covers_every_exchange_reader():
    found = exchange_readers()
    assert set(THE_FIVE) <= set(found) and "amph_party_partner_dev" in found and "amph_parties_partner_dev" in found
    check_exchange_matrix(found, EC.MATRIX)
    assert set(EC.MATRIX) == set(TC.LEFT_OUT) == set(THE_FIVE)
    assert all("exchange_cases.MATRIX" in reason for reason in TC.LEFT_OUT.values())
    for name, e in EC.MATRIX.items():
        assert e.on_rejection and e.modes and set(e.modes) <= {"host", "device"}, name
        assert ("device" in e.modes) == (name != "amph_exchange_decode_batch"), name  # the batch form is host-only


@pytest.mark.parametrize("gone", THE_FIVE)
def test_the_guard_fails_by_the_missing_name(gone):
    found = exchange_readers()
    short = {k: v for k, v in EC.MATRIX.items() if k != gone}
    with pytest.raises(AssertionError, match=r"%s(_dev)? \(\S+\) reads an exchange text" % gone):
        check_exchange_matrix(found, short)


def test_a_stale_key_is_refused():
    with pytest.raises(AssertionError, match="amph_gone is not a declaration"):
        check_exchange_matrix(exchange_readers(), dict(EC.MATRIX, amph_gone=EC.MATRIX["amph_exchange_decode"]))


def test_the_forms_are_the_gpu_file_s_parameters():
    """tests/test_hip_exchange_texts.py is a GPU module: its text is parsed, not imported."""
    src = open(os.path.join(ROOT, "tests", "test_hip_exchange_texts.py")).read()
    forms = re.findall(r'"(\w+)"', re.search(r"^FORMS = \[(.*?)\]", src, re.S | re.M).group(1))
    assert len(forms) == len(set(forms)) and set(forms) == {e.form for e in EC.MATRIX.values()}
    run = re.search(r"^RUN = \{(.*?)\}", src, re.S | re.M).group(1)
    assert set(re.findall(r'"(\w+)":', run)) == set(forms)
    assert re.search(r"^def form_parameters\(\):", src, re.M) and "EC.MATRIX" in src
    assert re.search(r'parametrize\("form,mode", form_parameters\(\)\)', src)


# ---- the two references and the declared verdicts ---------------------------------------------
def test_self_check_passes_for_every_case():
    seen = {}
    for cls in EC.CLASSES:  # (a builder may add a case of another class: the dense stretch beside the flood)
        for k, count in EC.self_check(EC.BUILDERS[cls]()).items():
            seen[k] = seen.get(k, 0) + count
    assert set(seen) == set(EC.CLASSES) and all(seen.values())
    assert len(EC.catalogue()) == sum(seen.values())


def json_pairs(text: bytes):
    """parse_pairs by Python's json module, arranged to be as strict as the header."""
    def constant(name):
        raise ValueError(name)
    try:
        s = text.decode("ascii")                          # strict ASCII
        if "\\" in s:                                     # a backslash form of a key is refused
            return None
        items = json.loads(s, parse_constant=constant, object_pairs_hook=lambda kv: ("object", kv))  # duplicates kept
    except ValueError:
        return None
    if type(items) is not list:
        return None
    out = []
    for it in items:
        if not (type(it) is tuple and len(it) == 2 and it[0] == "object"):
            return None
        kv = it[1]
        if sorted(k for k, _ in kv) != ["a", "b"] or any(type(v) is not int or abs(v) >= EC.TOP for _, v in kv):
            return None
        d = dict(kv)
        out.append((d["a"], d["b"]))
    return out


def test_parse_pairs_equals_python_s_json_on_every_text():
    refused = accepted = 0
    for c, e in EC.catalogue():
        assert e.parsed == json_pairs(c.text), c.name
        accepted += e.parsed is not None
        refused += e.parsed is None
    assert accepted > 1000 and refused > 1000
    for text in (b"[NaN]", b'[{"a":NaN,"b":1}]', b'[{"a":1,"b":Infinity}]', b'{"a":1,"b":2}', b"7", b"",
                 b'[{"a":1,"b":2,"a":1}]', b'[{"a":1}]', b'[{"\\u0061":1,"b":2}]', b"[[]]", b'[{"a":1,"b":2},]'):
        assert EC.parse_pairs(text) is None and json_pairs(text) is None, text
    assert EC.parse_pairs(b' [ ] ') == json_pairs(b' [ ] ') == []
    assert EC.parse_pairs(b'[{"b":-0,"a":%d}]' % (EC.TOP - 1)) == [(EC.TOP - 1, 0)]


# tests/test_wire.py's pinned offsets, as data: (text, pairs expected, offset)
_TWO = [
    (b'[{"a":1,"b":2},{"a":1.5,"b":2}]', 20), (b'[{"a":1,"b":2},{"a":1e5,"b":2}]', 20),
    (b'[{"a":1,"b":2},{"a":1,"a":2}]', 26), (b'[{"a":1,"b":2},{"a":1,"c":2}]', 26),
    (b'[{"a":1,"b":2},{"a":"1","b":2}]', 20), (b'[{"a":1,"b":2},{"a":1,"b":2,"a":3}]', 26),
    (b'[{"a":1,"b":2} {"a":1,"b":2}]', 20),
    (b'[{"a":1,"b":2},{"a":340282366920938463463374607431768211456,"b":2}]', 20),
    (b'[{"a":1,"b":2},{"a":--1,"b":2}]', 20), (b'[{"a":1,"b":2},{"a":01,"b":2}]', 20),
    (b'[{"a":1,"b":2},{"a":-00,"b":2}]', 20), (b'[{"a":1,"b":2}x,{"a":1,"b":2}]', 21),
    (b'[{"a":1,"b":2}}, {"a":1,"b":2}]', 22), (b'[{"a":1,"b":2},,{"a":1,"b":2}]', 21),
    (b'[{"a":1,"b":2},{"a":1,"b":2}x]', 26), (b'[{"a":1,"b":2},{"a":1,"b":2}]]', 26),
    (b'[{"a":1,"b":2},{"a":1,"b":2}] [', 26),
]
_MIDDLE = [
    (b'{"a":1.5,"b":2}', 20), (b'{"a":1e5,"b":2}', 20), (b'{"a":1,"a":2}', 26), (b'{"a":1,"c":2}', 26),
    (b'{"a":"1","b":2}', 20), (b'{"a":340282366920938463463374607431768211456,"b":2}', 20),
    (b'{"a":--1,"b":2}', 20), (b'{"a":01,"b":2}', 20), (b'{"a":-00,"b":2}', 20), (b'{"a":1,"b":-}', 26),
    (b'{"a":1,"b":2 }', -1), (b'{"a": 1,"b":2}', -1), (b'{"a":1,7,"b":2}', 28), (b'{"a":1,"b":2}5}', 36),
]
_EDGES = [(b'[x{"a":1,"b":2}]', 1, 7), (b'x[{"a":1,"b":2}]', 1, 0), (b'[{"a":1,"b":2}x]', 1, 12), (b'[ x ]', 0, 2),
          (b'[,]', 0, 1)]
PINNED = [(t, 2, at) for t, at in _TWO] + _EDGES + \
    [(b'[{"a":1,"b":2},' + m + b',{"a":7,"b":8},{"a":-9,"b":10}]', 4, at) for m, at in _MIDDLE]


def test_first_bad_reproduces_the_offsets_test_wire_pins():
    assert len(PINNED) == 17 + 5 + 14
    for text, npairs, at in PINNED:
        v = EC.first_bad(text, npairs)
        assert v == (EC.Verdict("ok", -1) if at < 0 else EC.Verdict("param", at)), (text, v, at)
        assert (EC.parse_pairs(text) is not None) == (at < 0), text
    # the count and the brackets (test_exchange_decode_count_and_brackets)
    assert EC.first_bad(b'[{"a":1,"b":2},{"a":3,"b":4}]', 3) == ("len", 29)
    assert EC.first_bad(b'{"a":1,"b":2},{"a":3,"b":4}]', 2).kind == "param"
    assert EC.first_bad(b"[]", 0) == ("ok", -1)
    # the stray-bytes tie at every pair of a longer text (test_exchange_decode_stray_bytes_between_pairs)
    pairs = EC.long_pairs(300, 5, 20)
    items = [b'{"a":%d,"b":%d}' % p for p in pairs]
    start = 1
    for k in range(len(items) - 1):
        where = start + len(items[k]) + len(b'5},{"a":')
        text = b"[" + b",".join(items[:k] + [items[k] + b"5}"] + items[k + 1:]) + b"]"
        assert EC.first_bad(text, len(pairs)) == ("param", where), k
        start += len(items[k]) + 1


def test_a_substitution_is_reported_within_one_entry_of_the_edit():
    """92 characters are one longest entry (kXEntry): whatever byte replaces whichever byte of a
    compact text, the reported token stands within that of the edit.  The brackets and the
    count verdict are exempt."""
    text = EC.compact([(-(EC.TOP - 1), -(EC.TOP - 2)), (1, 2), (-(EC.TOP - 3), 10 ** 38), EC.TEMPLATE, (0, -7),
                       (EC.TOP - 1, -(10 ** 38))])
    assert EC.first_bad(text, 6).kind == "ok" and len(text) > 3 * EC.ENTRY
    farthest = 0
    for at in range(1, len(text) - 1):
        for c in range(256):
            v = EC.first_bad(EC.poke(text, at, c), 6)
            if v.kind == "param":
                farthest = max(farthest, abs(v.bad - at))
                assert abs(v.bad - at) <= EC.ENTRY, (at, c, v)
    assert farthest > 40  # (the bound is not idle: a closing '}' gone is reported a whole member away)


# ---- coverage ---------------------------------------------------------------------------------
def test_the_coverage_the_catalogue_claims():
    full = EC.full_cases()
    positions = sum(len(r) for r in EC.SWEEPS.values())
    assert len(full) == 256 * positions and positions >= 60
    texts = {}
    for c in full:
        texts.setdefault(c.place, set()).add(c.text)
    for where, r in EC.SWEEPS.items():  # 256 byte values at every position: 255 other texts a position, and the honest one
        assert len(texts[where]) == 255 * len(r) + 1, where
    assert sum(c.want.kind == "ok" for c in full) > 60 * 3  # the substitutions the grammar accepts are kept
    assert {c.want.kind for c in full} == {"ok", "param", "len"}
    # every edge byte at every place (but the byte that stands there already)
    edge = EC.edge_cases()
    spots = EC.edge_places()
    assert set(EC.PLACES) == set(spots) | {"blanks257"} and len(EC.EDGE_BYTES) == 30
    at = {"border_8191": EC.SPAN - 1, "border_8192": EC.SPAN}
    for place, where in spots.items():
        assert len(where) == {"border_8191": 23, "border_8192": 23, "span1": 23, "first6": 6, "last2": 2}[place]
        for _, text, npairs, D, _, j in where:
            if place in at:
                assert D + j == at[place] and len(text) > EC.SPAN
            if place == "span1":
                assert len(text) >= EC.WINDOW_TEXT and EC.SPAN + 256 <= D + j < 2 * EC.SPAN - 256
            tried = {c.text[D + j] for c in edge if c.place == place and c.text[:D + j] == text[:D + j] and
                     c.text[D + j + 1:] == text[D + j + 1:]}
            assert tried == set(EC.EDGE_BYTES) - {text[D + j]}, (place, D, j)
    assert {c.text[6 + EC.BLANKS] for c in edge if c.place == "blanks257"} == set(EC.EDGE_BYTES) - {EC.MINUS}
    assert EC.BLANKS > 256
    # every digit count in every member role, at its least and greatest value, both signs
    numbers = EC.number_cases()
    for role in EC.ROLES:
        for nd in range(1, 40):
            got = [c for c in numbers if c.role == (nd, role) and c.want.kind == "ok"]
            assert len(got) >= 4, (role, nd)
    values = {v for c in numbers if c.want.kind == "ok" for p in EC.parse_pairs(c.text) for v in p}
    assert {EC.TOP - 1, 1 - EC.TOP, 10 ** 38, 0} <= values
    assert sum(c.name.startswith("number_border_") for c in numbers) == 40
    refused = [c for c in numbers if c.want.kind == "param"]
    assert len(refused) >= len(EC.ROLES) * len(EC.BAD_TOKENS)
    # a defect in span 1 of a text whose window lies inside it, in every class that has long texts
    # (FULL's texts hold three pairs)
    for cls in ("EDGE", "NUMBERS", "PAIRS"):
        assert any(len(c.text) >= EC.WINDOW_TEXT and EC.SPAN <= c.want.bad < 2 * EC.SPAN
                   for c in EC.BUILDERS[cls]() if c.want.kind == "param"), cls
    # what a session can hold, and what only the calls with a free pair count can
    assert all(EC.fits_a_session(c) for cls in ("EDGE", "NUMBERS", "ACCEPTED") for c in EC.BUILDERS[cls]())
    assert [c.name for c in EC.pair_cases() if not EC.fits_a_session(c)] == ["empty_one_pair_expected"]
    diagonal = EC.diagonal()
    assert {c.cls for c, _ in diagonal} == set(EC.CLASSES)
    assert {c.place for c, _ in diagonal} >= set(EC.PLACES)
    assert {c.role[0] for c, e in diagonal if c.role and e.kind == "ok"} == set(range(1, 40))
    assert {e.kind for _, e in diagonal} == {"ok", "param", "len"} and len(diagonal) < 200


# ---- the cases are decisive ---------------------------------------------------------------------
# the planted errors the catalogue must catch, in the issue's words
PLANTED = {
    "control_bytes_are_whitespace": "VT / FF / NUL taken as whitespace",
    "bit7_dropped": "bit 7 dropped before classifying: 0xBA reads as a colon, 0xB5 as a digit",
    "leading_zero": "a leading zero accepted",
    "forty_digits": "40 digits accepted",
    "wraps_at_2_128": "2^128 wrapped",
    "plus_sign": "'+' accepted",
    "lone_minus_is_zero": "a lone '-' taken as 0",
    "minus_zero_keeps_its_sign": "'-0' given a set sign byte",
    "same_key_twice": "the same key twice accepted",
    "opener_not_tied": "the opener not tied to the previous digit: '5}' passes",
    "bytes_after_the_bracket": "bytes after ']' accepted",
    "last_defect": "the last defect reported, not the first",
    "len_before_param": "E_LEN preferred over a malformed token",
    "offset_from_the_span": "the offset counted from the span start",
    "offset_from_the_aligned_base": "the offset counted from the aligned base, the misalignment not subtracted",
    "offset_from_the_buffer": "the offset counted from the packed buffer, not from the object",
}


def decisive_order():
    """The catalogue, the short texts first (a disagreement is usually found among them)."""
    return sorted(EC.catalogue(), key=lambda ce: len(ce[0].text))


def disagreements(flaw):
    """The cases on which the model with `flaw` planted differs from the catalogue, lazily."""
    slots = {}
    if flaw == "offset_from_the_buffer":  # the object's slot in the packed call's buffer
        at = 0
        for o in EC.objects("PAIRS+ACCEPTED"):
            slots[o.name] = at
            at += max(EC.SPAN, -(-len(o.text) // EC.SPAN) * EC.SPAN)
    for c, e in decisive_order():
        want = (EC.Verdict(e.kind, e.bad), EC.diffs_of(e.pairs) if e.pairs is not None else None)
        for mis in (EC.ALIGN if flaw == "offset_from_the_aligned_base" else (0,)):
            if EC.scan(c.text, c.npairs, flaw, mis=mis, slot=slots.get(c.name, 0)) != want:
                yield c.name, mis


def test_the_model_without_a_planted_error_equals_the_catalogue():
    assert next(disagreements(None), None) is None


@pytest.mark.parametrize("flaw", sorted(PLANTED))
def test_the_cases_are_decisive(flaw):
    assert flaw in EC.FLAWS, "%s (%s) is no longer a planted error of the model" % (flaw, PLANTED[flaw])
    assert next(disagreements(flaw), None) is not None, "no case notices: %s" % PLANTED[flaw]


def test_every_planted_error_is_listed():
    assert set(EC.FLAWS) == set(PLANTED)
    with pytest.raises(AssertionError):
        EC.scan(b"[]", 0, "no_such_flaw")
