"""The text catalogue (tests/text_cases.py) cannot rot -- all on the CPU.

* Every declaration of include/*.h that takes a `bad_char`, `bad_chars` or
  `bad_index` is a call of the text matrix (TC.MATRIX) or is left out with a
  reason (TC.LEFT_OUT); no key is stale; every form the matrix names is a
  parameter of tests/test_hip_texts.py.  The prototype parser is that of
  tests/test_session_cases_cpu.py, tested here on the new parameter names.
* The catalogue's declared verdicts equal `first_bad` recomputed from the
  edited text (TC.self_check, at every size, party count and kind), `first_bad`
  equals a byte-by-byte restatement of itself, and the coverage it claims is
  there: FULL holds 256 x positions, LATIN 64 x positions, every edge byte,
  every place and every (place, class) occurs, the diagonal keeps them.
* A Python model of the decoder equals the catalogue, and with ONE planted
  error each it disagrees with it on at least one case: the cases are decisive.
"""
import base64
import os
import re

import pytest

from tests import field_cases as FC
from tests import text_cases as TC
from tests import verdict_cases as VC
from tests.test_session_cases_cpu import declarations_with, prototypes_with

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXT_VERDICT = r"bad_chars?|bad_index"


# ---- the text matrix covers the headers -------------------------------------------------------
def test_the_parser_finds_the_three_spellings_and_nothing_else():
    text = """
    int amph_one(amph_ctx* ctx, const char* in, int64_t* bad_index, uint32_t flags);
    int amph_two(amph_s* s, uint8_t* out, int64_t* first_fail,
                 int64_t *bad_char, void* stream);
    int amph_many(amph_s* s, int64_t* first_fails, int64_t* bad_chars);
    /* int amph_commented(amph_ctx* ctx, int64_t* bad_char); */
    int amph_other(amph_ctx* ctx, int64_t* bad_character, int64_t* bad_indexes);
    int amph_none(amph_ctx* ctx, int64_t* first_fail);
    int amph_not_a_pointer(amph_ctx* ctx, int64_t bad_index);
    """
    assert prototypes_with(text, TEXT_VERDICT) == ["amph_one", "amph_two", "amph_many"]


def check_text_matrix(found, matrix, left_out):
    assert not set(matrix) & set(left_out)
    assert all(left_out.values())  # a written reason each
    known = set(matrix) | set(left_out)
    for name, header in found.items():
        base = name[:-4] if name.endswith("_dev") else name
        assert name in known or base in known, "%s (%s) takes a text verdict and is in no text test" % (name, header)
    for name in known:  # no stale key
        assert name in found, "%s is not a declaration with a bad_char, bad_chars or bad_index" % name
    for name in found:  # the _dev siblings run through their base names: the base is declared too
        if name.endswith("_dev"):
            assert name[:-4] in found, name


def test_the_text_matrix_covers_every_text_verdict():
    found = declarations_with(TEXT_VERDICT)
    assert len(found) >= 36 and "amph_base64_decode" in found and "amph_clients_finish_mask_json_dev" in found
    assert "amph_convert_share_json_batch" in found and "amph_parties_partner_dev" in found
    check_text_matrix(found, TC.MATRIX, TC.LEFT_OUT)
    assert all(e.kind in ("field", "record", "data", "stream") and e.on_rejection for e in TC.MATRIX.values())


def test_the_text_guard_fails_by_the_missing_call_s_name():
    found = declarations_with(TEXT_VERDICT)
    for gone, header in (("amph_convert_share_json", "amphora.h"), ("amph_clients_party", "amphora_client_batch.h")):
        short = {k: v for k, v in TC.MATRIX.items() if k != gone}
        with pytest.raises(AssertionError, match=r"%s \(%s\) takes a text verdict" % (gone, re.escape(header))):
            check_text_matrix(found, short, TC.LEFT_OUT)
    with pytest.raises(AssertionError, match="amph_gone is not a declaration"):
        check_text_matrix(found, dict(TC.MATRIX, amph_gone=TC.MATRIX["amph_base64_decode"]), TC.LEFT_OUT)


def test_the_text_matrix_forms_are_the_tests_parameters():
    """tests/test_hip_texts.py is a GPU module: its text is parsed, not imported."""
    src = open(os.path.join(ROOT, "tests", "test_hip_texts.py")).read()
    lists = {}
    for name in ("FULL_IMPLS", "PACKED_FORMS", "DIAGONAL_FORMS"):
        m = re.search(r"^%s = \[(.*?)\]" % name, src, re.S | re.M)
        lists[name] = re.findall(r'"(\w+)"', m.group(1))
    forms = lists["PACKED_FORMS"] + lists["DIAGONAL_FORMS"]
    assert len(forms) == len(set(forms)) and set(forms) == {e.form for e in TC.MATRIX.values()}
    assert lists["PACKED_FORMS"] == list(TC.PACKED_FORMS) and lists["FULL_IMPLS"] == list(TC.IMPLS) == list(TC.DECIDERS)
    run = re.search(r"^RUN = \{(.*?)\}", src, re.S | re.M).group(1)
    packed = re.search(r"^RUN_PACKED = \{(.*?)\}", src, re.S | re.M).group(1)
    assert set(re.findall(r'"(\w+)":', run)) == set(lists["DIAGONAL_FORMS"])
    assert set(re.findall(r'"(\w+)":', packed)) == set(lists["PACKED_FORMS"])
    for impl in lists["FULL_IMPLS"]:  # each implementation's FULL and LATIN run is a parameter of a test
        assert re.search(r'parametrize\("impl", \[[^\]]*"%s"' % impl, src), impl


# ---- the reference ----------------------------------------------------------------------------
def plain_first_bad(text, kind):
    """first_bad byte by byte, from the rule's words."""
    n = len(text)
    for i, c in enumerate(text):
        if kind == "field":
            ok = c in TC.ALPHABET if i < n - TC.field_pad(n) else c == TC.EQ
        elif kind == "stream":
            ok = c in TC.ALPHABET or (c == TC.EQ and (i == n - 1 or (i == n - 2 and text[n - 1] == TC.EQ)))
        elif kind == "record":
            ok = c in TC.ALPHABET if i % 24 < 22 else c == TC.EQ
        else:
            r, f = divmod(i - 1, 37)
            last = r == (n - 1) // 37 - 1
            frame = b'{"value":"' + bytes(24) + b'"}' + (b"]" if last else b",")
            ok = c == ord("[") if i == 0 else (c in TC.ALPHABET if 10 <= f < 32 else c == TC.EQ if f in (32, 33)
                                               else c == frame[f])
        if not ok:
            return i
    return -1


def test_first_bad_equals_its_plain_restatement():
    for kind in ("record", "data", "stream"):
        text = TC.single_text(kind)
        assert TC.first_bad(text, kind) == plain_first_bad(text, kind) == -1
        cases = TC.single_diagonal(kind) + TC.single_pairs(kind)
        for c in cases:
            t = TC.edited_single(text, c)
            assert TC.first_bad(t, kind) == plain_first_bad(t, kind) == c.want >= 0, (kind, c.name)
    for W in TC.SIZES:
        b, cs = TC.catalogue("test", 3, W, "diagonal+pairs+accepted")
        for c, e in cs:
            for (j, k), t in TC.apply(b, c).items():
                assert TC.first_bad(t, "field") == plain_first_bad(t, "field"), (W, c.name)


def test_accepted_texts_decode_as_python_decodes_them():
    for kind in ("record", "data", "stream"):
        text = TC.single_text(kind)
        words = TC.record_words() if kind != "stream" else TC.record_words(TC.W_FULL, "text_cases/stream")
        assert TC.words_of(TC.decoded(text, kind)) == list(words)
    # the unused low bits of a record's last data character are ignored
    rec = bytearray(VC.record(5))
    rec[21] = TC.ALPHABET[TC.ALPHABET.index(rec[21]) | 15]
    assert TC.first_bad(bytes(rec), "record") == -1 and TC.words_of(TC.decoded(bytes(rec), "record")) == [5]
    assert base64.b64decode(bytes(rec)) == (5).to_bytes(16, "little")


# ---- the catalogue ---------------------------------------------------------------------------------
def test_the_sizes_reach_every_padding_and_lane_kind():
    pads = {}
    for W in TC.SIZES:
        n = TC.wire_chars(W)
        pad = TC.field_pad(n)
        pads.setdefault(pad, []).append(W)
        assert n % 16 == {2: 8, 1: 12, 0: 0}[pad]
        # the tile that holds the text's end: at least one fast lane, exactly one per-character unit
        last_tile = (n - 1) // TC.TILE_CHARS
        units = range(last_tile * 256, (n + 15) // 16)
        fast = [u for u in units if 16 * (u + 1) + 4 <= n]
        assert fast and len(units) - len(fast) == 1 and fast[-1] == TC.border_unit(n), W
        P = TC.places(W)
        assert P["border_a"] == 16 * fast[-1] + 15 and P["border_b"] == P["border_a"] + 1
        assert P["last_data"] == n - pad - 1 and [P["pad%d" % i] for i in range(pad)] == list(range(n - pad, n))
        assert ("tile_a" in P) == (n > TC.TILE_CHARS) == (W >= 193)
    assert all(any(W < 193 for W in ws) and any(W >= 193 for W in ws) for ws in pads.values()) and set(pads) == {0, 1, 2}


def test_the_stream_text_takes_the_block_kernel():
    """One whole 256-unit block for k_b64_decode_blk and a last workgroup of one whole unit and a
    padded one; the field text of the same size has a fast tile and a per-character one."""
    n = len(TC.single_text("stream"))
    units = (n + 15) // 16
    assert n == TC.wire_chars(TC.W_FULL) and (units - 1) // 256 == 1 and units == 258 and TC.field_pad(n) == 2
    assert TC.TILE_CHARS + 4 <= n < 2 * TC.TILE_CHARS + 4  # wire.hip: tile 0 is fast, tile 1 is not
    for impl in ("stream_block", "wire_fast"):
        assert {TC.IMPLS[impl].unit(v, q) for v in range(256) for q in range(16)} <= set(range(256))
    assert TC.IMPLS["stream_tail"].unit(0, 0) == 256 == TC.IMPLS["wire_last"].unit(0, 0)
    assert {TC.IMPLS["convert_json"].unit(v, q) for v in range(256) for q in range(22)} == set(range(TC.RECORDS))


@pytest.mark.parametrize("impl", list(TC.IMPLS))
def test_full_and_latin_hold_every_pair(impl):
    I = TC.IMPLS[impl]
    for n in (TC.PARTIES if I.kind == "field" else (1,)):
        cases = TC.full_cases(impl, n)
        pairs = {(c.edits[0][3], q) for c in cases for q in range(I.positions)
                 if c.edits[0][2] == TC.impl_offset(impl, I.unit(c.edits[0][3], q), q)}
        assert len(cases) == len(pairs) == 256 * I.positions
        assert sum(c.want == -1 for c in cases) == 64 * I.positions
        if I.kind == "field":
            b = VC.base("test", n, TC.W_FULL)
            TC.self_check(b, cases)
            latin = TC.latin_cases(impl, n)
            assert len(latin) == (64 if impl == "wire_last" else 1)
            for c in latin:
                e = TC.expect(b, c)
                # the words change, and with them the MACs; a row in a y field changes the secrets too
                assert e.bad == -1 and e.ff >= 0 and bool(e.changed) == (c.edits[0][1] == VC.Y), c.name
            assert len({(v, at % 16) for c in latin for _, _, at, v in c.edits}) == 64 * 16
        else:
            TC.single_self_check(I.kind, cases)
    rows = TC.latin_rows(impl)
    assert len({(row[q], q) for _, row in rows for q in range(I.positions)}) == 64 * I.positions
    assert all(set(row) <= set(TC.ALPHABET) for _, row in rows)
    if I.kind != "field":
        text = TC.single_text(I.kind)
        texts = TC.latin_texts(impl, text)
        assert len(texts) == (64 if impl == "stream_tail" else 1)
        for t in texts:
            assert TC.first_bad(t, I.kind) == -1 and TC.decoded(t, I.kind) != TC.decoded(text, I.kind)


@pytest.mark.parametrize("n", TC.PARTIES)
def test_the_catalogue_checks_itself_and_covers_what_it_claims(n):
    for pid in TC.PRIMES:
        for W in TC.SIZES:
            which = "edge+pairs+accepted" if pid == "test" else "accepted"  # rejection does not depend on the field
            b, cs = TC.catalogue(pid, n, W, which)
            seen = TC.self_check(b, [c for c, _ in cs])
            assert seen["ACCEPTED"] == (2 if TC.field_pad(TC.wire_chars(W)) else 1)
            if pid != "test":
                continue
            edge = [c for c, _ in cs if c.cls == "EDGE"]
            P = TC.places(W)
            assert {c.place for c in edge} == set(P) and {c.edits[0][3] for c in edge} >= set(TC.EDGE_BYTES)
            for name in P:
                at_place = [c for c in edge if c.place == name]
                assert {c.edits[0][3] for c in at_place} == set(TC.place_bytes(name))
                assert {TC.byte_class(c.edits[0][3]) for c in at_place} == set(TC.place_classes(name))
                assert all(c.edits[0][2] == P[name] for c in at_place)
            assert TC.EQ in TC.place_bytes("mid") and TC.EQ in TC.place_bytes("last_data")  # '=' in mid-text, at the end
            assert {(j, k) for c in edge for j, k, _, _ in c.edits} == {(j, k) for j in range(n) for k in range(5)}
            # the diagonal: each byte once at least, each (place, class), each place twice
            diag = TC.diagonal(n, W)
            assert {c.edits[0][3] for c in diag} >= set(TC.EDGE_BYTES) and len(diag) < len(edge) // 4
            for name in P:
                at_place = [c for c in diag if c.place == name]
                assert len(at_place) >= 2
                assert {TC.byte_class(c.edits[0][3]) for c in at_place} == set(TC.place_classes(name))
            names = {c.name for c, _ in cs}
            assert {"pair_high_then_ascii", "pair_ascii_then_high", "pair_c1_then_ascii", "pair_two_dwords"} <= names
            assert ("pair_two_tiles" in names) == (W >= 193) and ("pair_party_major" in names) == (n >= 3)
            assert ("pair_with_mac_fault" in names) == (W >= 2)
    # the MAC fault alone is a fault: the text verdict outranks something
    b, cs = TC.catalogue("test", n, 193, "pairs")
    c = next(c for c, _ in cs if c.name == "pair_with_mac_fault")
    alone = TC.expect(b, TC.Case("mac_alone", "PAIR", (), c.word_edits, -1, None))
    assert alone == TC.Expect(-1, 192, {})


def test_the_packed_objects_hold_every_size_and_clean_neighbours():
    P = TC.packed_objects("test", 3)
    assert set(P.sizes) == set(TC.SIZES) and len(P.objects) > 2000
    clean = [i for i, o in enumerate(P.objects) if o.case is TC.HONEST]
    assert all(P.objects[i - 1].case is not TC.HONEST for i in clean)  # a clean object after every third case
    assert all(b - a <= 6 for a, b in zip(clean, clean[1:])) and clean[0] == 3
    assert all(x % 16 == 0 for x in P.foff) and P.woff[-1] == sum(P.sizes)
    refused = [o for o in P.objects if o.expect.bad >= 0]
    assert {o.case.cls for o in refused} == {"EDGE", "PAIR"} and all(o.expect.ff is None for o in refused)


def test_the_single_text_cases_cover_their_places():
    for kind in ("record", "data", "stream"):
        P = TC.single_places(kind)
        cases = TC.single_edge_cases(kind)
        TC.single_self_check(kind, cases + TC.single_pairs(kind))
        diag = TC.single_diagonal(kind)
        assert {c.edits[0][3] for c in diag} >= set(TC.EDGE_BYTES)
        for name, (at, tried, classes, want) in P.items():
            got = [c for c in diag if c.place == name]
            assert len(got) >= 2 and {TC.byte_class(c.edits[0][3]) for c in got} == set(classes), (kind, name)
    assert {"r127_q15", "r128_q0", "r128_q23", "r0_open", "r128_sep", "lead"} <= set(TC.single_places("data"))


# ---- a Python model of the decoder, with one planted error each ---------------------------------------
BUGS = {
    "accept_dash": "'-' and '_' (the URL-safe alphabet) read as '+' and '/'",
    "accept_at": "'@', one below 'A', is in the alphabet",
    "accept_bracket": "'[', one above 'Z', is in the alphabet",
    "accept_backtick": "'`', one below 'a', is in the alphabet",
    "accept_brace": "'{', one above 'z', is in the alphabet",
    "accept_colon": "':', one above '9', is in the alphabet",
    "accept_dot": "'.', one below '/', is in the alphabet",
    "drop7": "bit 7 is dropped before the lookup: 0xC1 reads as 'A'",
    "eq_anywhere": "'=' is accepted outside the padding",
    "pad_unchecked": "the padding positions are not looked at",
    "last_of_unit": "the last offender of a unit is reported instead of the first",
    "field_major": "of several fields the smallest (field, party) wins, not the smallest (party, field)",
    "high_hides": "a byte >= 0x80 is judged by its low 7 bits and lets the next byte of its dword pass",
    "skip_first_slow_lane": "the first per-character lane of the text's last tile is not decoded",
}
_ACCEPTS = {"accept_dash": b"-_", "accept_at": b"@", "accept_bracket": b"[", "accept_backtick": b"`",
            "accept_brace": b"{", "accept_colon": b":", "accept_dot": b".", "eq_anywhere": b"="}


def model_char_ok(c, bug):
    if bug in ("drop7", "high_hides"):
        c &= 0x7F
    if c in _ACCEPTS.get(bug, b""):
        return True
    return 0x41 <= c <= 0x5A or 0x61 <= c <= 0x7A or 0x30 <= c <= 0x39 or c == 0x2B or c == 0x2F


def model_text(t, honest, bug):
    """The first offender of one field text, unit by unit (16 characters a lane), or -1.  Only
    the units that differ from the honest text and the one that holds the padding are looked
    at: the honest text passes under every planted error (asserted by the caller)."""
    n = len(t)
    pad = TC.field_pad(n)
    slow = TC.border_unit(n) + 1
    for u in range((n + 15) // 16):
        lo, hi = 16 * u, min(16 * u + 16, n)
        if t[lo:hi] == honest[lo:hi] and hi <= n - pad:
            continue
        if bug == "skip_first_slow_lane" and u == slow:
            continue
        offenders = []
        for pos in range(lo, hi):
            if pos >= n - pad:
                ok = bug == "pad_unchecked" or t[pos] == TC.EQ
            else:
                ok = model_char_ok(t[pos], bug)
                if bug == "high_hides" and pos % 4 and t[pos - 1] >= 0x80:
                    ok = True
            if not ok:
                offenders.append(pos)
        if offenders:
            return offenders[-1] if bug == "last_of_unit" else offenders[0]
    return -1


def model_call(b, case, bug=None):
    """bad_char of a whole call: every party's every field, the smallest code."""
    honest = TC.field_texts(b)
    nc = TC.wire_chars(b.W)
    hits = []
    for (j, k), t in TC.apply(b, case).items():
        at = model_text(t, honest[j][k], bug)
        if at >= 0:
            hits.append((j, k, at))
    if not hits:
        return -1
    j, k, at = min(hits, key=(lambda h: (h[1], h[0], h[2])) if bug == "field_major" else None)
    return TC.code(nc, j, k, at)


def test_the_honest_texts_pass_under_every_planted_error():
    for W in TC.SIZES:
        for t in TC.field_texts(VC.base("test", 3, W))[0]:
            for bug in [None] + list(BUGS):
                assert model_text(t, b"", bug) == -1 or bug == "skip_first_slow_lane"
                assert all(model_char_ok(c, bug) for c in t[:len(t) - TC.field_pad(len(t))])


@pytest.mark.parametrize("bug", list(BUGS))
def test_every_planted_error_is_caught(bug):
    """The unplanted model equals the catalogue on every case; the planted one differs on one
    at least -- on the catalogue's verdicts alone, no library call."""
    caught = []
    for W in TC.SIZES:
        b, cs = TC.catalogue("test", 3, W)
        for c, e in cs:
            assert model_call(b, c) == e.bad, (W, c.name)
            if model_call(b, c, bug) != e.bad:
                caught.append((W, c.name))
    assert caught, (bug, BUGS[bug])
    if bug == "field_major":
        assert {name for _, name in caught} == {"pair_party_major"}
    if bug == "high_hides":  # 0xC1 then '*' in one dword: neither is seen
        assert any(name == "pair_c1_then_ascii" for _, name in caught)
    if bug == "skip_first_slow_lane":
        assert any("border_b" in name for _, name in caught)


def test_the_full_cases_catch_the_alphabet_errors():
    """FULL alone (one unit, 256 values) catches every planted error about single characters."""
    b = VC.base("test", 1, TC.W_FULL)
    cases = TC.full_cases("wire_last", 1)
    for bug in list(_ACCEPTS) + ["drop7"]:
        assert any(model_call(b, c, bug) != c.want for c in cases), bug
    assert all(model_call(b, c) == c.want for c in cases)
    assert FC.BY_ID["test"].big and not FC.BY_ID["m89"].big
