"""The buffer-extent harness (tests/extent_cases.py) must be able to fail:
numpy stand-ins for a callee, each with one planted error, are rejected by
the check that error breaks; the placement rules hold; and the table of calls
covers include/amphora.h.  No GPU."""
import os
import re

import numpy as np
import pytest

from tests import extent_cases as X
from tests.test_abi import header_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORDS = np.arange(64, dtype=np.uint8) + 1  # four 16-byte words


def plan(check=None):
    """A callee that copies four words: out = a."""
    out = X.Arr("out", X.WORD, n=64, expect=None if check else WORDS.tobytes())
    return X.Plan("copy", [X.Arr("a", X.WORD, data=WORDS)], [out, X.Arr("ff", X.VERDICT, verdict=-1)], None,
                  check=check)


def good(ins, outs):
    outs["out"].view[:] = ins["a"].view
    outs["ff"].view[:] = np.frombuffer(X.le8(-1, signed=True), np.uint8)
    return X.OK


def planted(edit):
    def callee(ins, outs):
        st = good(ins, outs)
        edit(ins, outs)
        return st
    return callee


def test_a_correct_callee_passes():
    got = X.run_plan(plan(), False, good)
    assert got["out"] == WORDS.tobytes()


def _poke(which, rel, n=1):
    """Write n bytes at payload offset rel of an array (bands are reachable)."""
    def edit(ins, outs):
        g = (outs if which in outs else ins)[which]
        g.region[g.lo + rel: g.lo + rel + n] ^= 0x5A
    return edit


@pytest.mark.parametrize("edit,message", [
    (_poke("out", -1), r"out \(word, 64 bytes\): band byte at payload offset -1 changed"),
    (_poke("out", 64), r"out \(word, 64 bytes\): band byte at payload offset 64 changed"),
    (_poke("out", 64, 16), r"band byte at payload offset 64 changed"),      # a 16-byte store one word past the end
    (_poke("ff", 8), r"ff \(verdict, 8 bytes\): band byte at payload offset 8 changed"),
    (_poke("a", 5), r"input a \(word, 64 bytes\): byte at payload offset 5 changed"),
    (_poke("a", -200), r"input a .* byte at payload offset -200 changed"),
    (_poke("a", 64 + 255), r"input a .* byte at payload offset 319 changed"),
    (_poke("out", 3), r"output out differs from the reference at byte 3 of 64"),
], ids=["byte-before", "byte-after", "word-past-end", "verdict-band", "input-payload", "input-front-band",
        "input-back-band", "wrong-output"])
def test_each_planted_error_is_rejected(edit, message):
    with pytest.raises(AssertionError, match=message):
        X.run_plan(plan(), False, planted(edit))


def test_wrong_status_and_verdict_are_rejected():
    with pytest.raises(AssertionError, match="status 1, expected 0"):
        X.run_plan(plan(), False, lambda i, o: good(i, o) or X.E_VERIFY)

    def verdict(ins, outs):
        good(ins, outs)
        outs["ff"].view[:] = np.frombuffer(X.le8(X.NF), np.uint8)  # the device sentinel in a host word
        return X.OK
    with pytest.raises(AssertionError, match="output ff differs"):
        X.run_plan(plan(), False, verdict)


def consume_one_past_the_end(ins, outs):
    """A tail lane that folds the byte after the input into the last output byte."""
    a = ins["a"]
    good(ins, outs)
    outs["out"].view[63] ^= a.region[a.lo + a.n]
    return X.OK


def test_an_output_that_depends_on_the_surroundings_is_rejected():
    # with a reference, P1 catches it in S1 (S0's zeros are harmless: the luck the issue describes)
    with pytest.raises(AssertionError, match=r"copy \[S1\]: output out differs from the reference at byte 63"):
        X.run_plan(plan(), False, consume_one_past_the_end)
    # where the reference is a property of the outputs that still holds, P4 names the dependency
    with pytest.raises(AssertionError, match="output out depends on the bytes around the inputs"):
        X.run_plan(plan(check=lambda got: None), False, consume_one_past_the_end)


def test_hostile_bytes_touch_both_ends():
    for kind, first, last in ((X.WORD, 0xFF, 0xFF), (X.SIGN, 0xFF, 0xFF), (X.XCHG, ord(":"), ord(":")),
                              (X.B64, None, ord("!")), (X.JSONTXT, ord('"'), ord(","))):
        g = X.guard(kind, data=b"[]" * 8, fill="hostile", offset=5 if kind in (X.XCHG, X.JSONTXT) else None)
        r = g.region
        if first is not None:
            assert r[g.lo - 1] == first, kind
        assert r[g.lo + g.n] == last, kind
        bands = np.concatenate([r[:g.lo], r[g.lo + g.n:]])
        assert not (bands == 0).any()
    g = X.guard(X.XCHG, data=b"[]", fill="hostile")
    assert g.region[:g.lo].tobytes().endswith(b',{"a":1,"b":2}:')
    assert g.region[g.lo + 2:].tobytes().startswith(b':,{"a":1,"b":2},{"a":1,"b":2}')
    assert set(X.guard(X.B64, data=b"AAAA", fill="hostile").region[:64].tolist()) == {ord("!"), ord("="), 0xFF}
    z = X.guard(X.WORD, data=WORDS, fill="zeros")
    assert not z.region[:z.lo].any() and not z.region[z.lo + 64:].any()


def test_the_pattern_has_no_blank_or_sentinel():
    """A band byte never equals a value the library writes as a blank or a
    sentinel, so such a byte stored into a band always changes it: checked
    for 0x20 (and the rest of FORBIDDEN) at every band position."""
    p = X.band_pattern(0, 1 << 16)
    assert not np.isin(p, X.FORBIDDEN).any()
    assert len(set(p[:256].tolist())) >= 256 - len(X.FORBIDDEN)  # position-dependent: no short period
    assert not np.array_equal(p[:4096], p[16:4096 + 16]) and not np.array_equal(p[:4096], p[1:4097])
    for blank in X.FORBIDDEN:
        g = X.guard(X.WORD, n=64)
        for rel in list(range(-g.lo, 0)) + list(range(64, 64 + X.BAND)):
            g.region[:] = g.before
            g.region[g.lo: g.lo + 64] = WORDS       # a correct payload
            g.region[g.lo + rel] = blank
            g.arena.fetch()
            with pytest.raises(AssertionError, match="payload offset %d changed" % rel):
                g.check_untouched()


def test_placement_rules():
    a = X.Arena(False)
    w = a.add("w", X.WORD, n=160)
    r = a.add("r", X.REC24, n=48)
    s = a.add("s", X.SIGN, n=6)
    v = a.add("v", X.VERDICT, n=8)
    o = a.add("o", X.OFFS, n=24)
    b = a.add("b", X.B64, n=24)
    texts = [a.add("t%d" % k, X.XCHG, n=13, offset=k) for k in range(16)]
    a.commit()
    assert w.ptr % 32 == 16 and w.ptr % 256 == 48       # 16-aligned, not 32- or 256-aligned
    assert r.ptr % 16 == 8
    assert s.ptr % 16 == 2
    assert v.ptr % 16 == 8 and o.ptr % 16 == 8
    assert b.ptr % 32 == 16
    assert [t.ptr % 16 for t in texts] == list(range(16))
    items = sorted(a.items, key=lambda g: g.start)
    for g in items:
        assert g.lo >= X.BAND and g.size - g.lo - g.n >= X.BAND and (a.base + g.start) % 256 == 0
    for g, h in zip(items, items[1:]):
        assert g.start + g.size <= h.start               # regions never overlap
    assert items[-1].start + items[-1].size <= a.size


def _prototypes():
    src = open(os.path.join(ROOT, "include", "amphora.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(amph_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, re.S)}


def test_the_table_covers_the_header():
    names = header_functions()
    table = X.table_names()
    assert not set(table) & set(X.LEFT_OUT)
    assert sorted(table + list(X.LEFT_OUT)) == names       # every symbol: an entry, or a reason
    assert all(X.LEFT_OUT.values())
    for must in ("amph_verify_message", "amph_mask_word_host"):
        assert must in X.LEFT_OUT
    modes = {}
    for c in X.CALLS:
        for n in c.names:
            modes.setdefault(n, set()).update(c.modes)
    protos = _prototypes()
    for name, args in protos.items():
        if "flags" in args and not name.endswith("_batch"):  # takes AMPH_F_DEVICE: both modes
            assert modes[name] == {"device", "host"}, name
        elif name.endswith("_batch"):
            assert modes[name] == {"host"}, name
    for name in ("amph_synth_odos", "amph_synth_words", "amph_stream_probe", "amph_party_begin_dev",
                 "amph_party_partner_dev", "amph_party_finish_b64_dev"):
        assert modes[name] == {"device"}, name
    # every host call that writes a caller array: a non-const pointer argument other than the handles
    for name, args in protos.items():
        writes = [a for a in args.split(",") if "*" in a and "const" not in a
                  and not re.search(r"amph_(ctx|party|stats)\b|\bvoid\s*\*", a)]
        if writes and name not in X.LEFT_OUT:
            assert name in modes, name
        if name in X.LEFT_OUT:
            assert not [a for a in writes if "uint8_t*" in a or "int64_t*" in a] or \
                name in ("amph_verify_message", "amph_mask_word_host"), name


def test_header_citations_name_their_calls():
    lines = open(os.path.join(ROOT, "include", "amphora.h")).read().split("\n")
    for c in X.CALLS:
        text = ""
        for part in c.header.split(","):
            lo, _, hi = part.strip().partition("-")
            assert 1 <= int(lo) <= int(hi or lo) <= len(lines), c.id
            text += "\n".join(lines[int(lo) - 1:int(hi or lo)])
        assert any(n in text for n in c.names), (c.id, c.header)


def test_every_entry_yields_its_sizes():
    d = X.data("test")
    for c in X.CALLS:
        labels = [p.label for p in c.gen(d)]
        assert labels and len(set(labels)) == len(labels), c.id
        if c.lane:
            strided = [p.label for p in c.gen(d, strided=True)]
            for W in X.STRIDE_SIZES:
                assert any(re.search(r"=%d\b" % W, s) for s in strided), (c.id, W)
            for W in X.LANE_SIZES:
                assert any(re.search(r"=%d\b" % W, s) for s in labels), (c.id, W)
