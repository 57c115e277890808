"""Response bodies for the body calls of include/amphora_client_bodies.h: a
builder that puts the five base64 members anywhere in a VerifiableSecretShare
JSON body (order, spacing, tags, padding in front of the first member), the
scanner's catalogue -- plain bodies with the reference's spans from
wire.odo_field_texts, and one group of bodies per refusal class -- and a plain
Python model of the scanner with ONE planted error each.  Shared by
tests/bodies/test_clients_bodies_cpu.py and tests/bodies/test_clients_bodies.py.
"""
import base64
import struct
from collections import namedtuple

NAMES = ("secretShares", "rShares", "vShares", "wShares", "uShares")
OK, NO_OBJECT, MISSING, NOT_STRING, TWICE, ESCAPE, UNTERMINATED = range(7)  # amph::BodyScan
REASONS = {NO_OBJECT: "no enclosing object", MISSING: "a member is missing",
           NOT_STRING: "a member is null or not a string", TWICE: "a member is given twice",
           ESCAPE: "a backslash inside a member's value", UNTERMINATED: "an unterminated string"}
SID = "00000000-0000-0000-0000-00000000002a"

# tags as raw JSON text: keys and values with \" and \\" (an escaped backslash in front of the closing
# quote), the members' own names as tag keys, tag values and NESTED keys, braces and brackets, non-ASCII
TAGS = {
    "none": '[]',
    "plain": '[{"key":"k","value":"v","valueType":"STRING"}]',
    "quotes": '[{"key":"a\\"b","value":"c\\\\\\"d\\\\","valueType":"STRING"},'
              '{"key":"q","value":"e\\"}]{","valueType":"STRING"}]',
    "names": '[{"key":"rShares","value":"uShares","valueType":"STRING"},{"key":"k","value":"\\"secretShares\\":\\"AAAA\\"",'
             '"valueType":"STRING"}]',
    "nested": '[{"key":"k","value":"v","rShares":"bm90IGEgbWVtYmVy","wShares":null,"valueType":"STRING"}]',
    "braces": '[{"key":"}{][","value":"]}\\"}{[","valueType":"STRING"},[[{"uShares":"{"}]]]',
    "unicode": '[{"key":"ключ","value":"值 \U0001F511 é","valueType":"STRING"}]',
}


def text_of(W, seed=0):
    """The base64 text of W 16-byte words (bytes); any W, its '=' padding included."""
    raw = bytes((seed * 131 + 7 * i + (i >> 8)) & 0xFF for i in range(16 * W))
    return base64.b64encode(raw)


def body(texts, order=(0, 1, 2, 3, 4), pretty=False, tags="plain", tags_at="first", pad=0, sid=SID):
    """A VerifiableSecretShare body (str) with the five member texts (bytes or
    str) in `order`; `pad` spaces stand in front of the first member, so
    every member moves by one byte per pad; tags_at: first / middle / last."""
    t = [x.decode("latin-1") if isinstance(x, (bytes, bytearray)) else x for x in texts]
    sep, colon = (",\n  ", " : ") if pretty else (",", ":")
    members = ['"%s"%s"%s"' % (NAMES[k], colon, t[k]) for k in order]
    meta = ['"secretId"%s"%s"' % (colon, sid), '"tags"%s%s' % (colon, TAGS.get(tags, tags))]
    members[0] = " " * pad + members[0]
    if tags_at == "first":
        parts = meta + members
    elif tags_at == "last":
        parts = members + meta
    else:
        parts = members[:2] + meta + members[2:]
    return ("{\n  " if pretty else "{") + sep.join(parts) + ("\n}" if pretty else "}")


def reference_spans(text):
    """(starts, lens) in BYTES of the UTF-8 body, from wire.odo_field_texts."""
    from amphora_amd import wire
    vals, spans = wire.odo_field_texts(text)
    starts, lens = [], []
    for v, (_, e) in zip(vals, spans):
        at = e - 1 - len(v)  # the closing quote stands at e - 1
        starts.append(len(text[:at].encode("utf-8")))
        lens.append(len(v.encode("utf-8")))
    return starts, lens


ScanCase = namedtuple("ScanCase", "name body expect")  # body: str; expect: OK or the refusal class


def rotations():
    return [tuple((r + k) % 5 for k in range(5)) for r in range(5)]


def plain_cases():
    out = []
    for W in (0, 1, 2, 3):
        texts = [text_of(W, seed=10 * W + k) for k in range(5)]
        for pretty in (False, True):
            for order in rotations():
                for tags in TAGS:
                    at = ("first", "middle", "last")[(order[0] + len(tags)) % 3]
                    out.append(ScanCase("W%d-%s-rot%d-%s-%s" % (W, "pretty" if pretty else "compact", order[0], tags, at),
                                        body(texts, order, pretty, tags, at, pad=(order[0] * 3 + W) % 16), OK))
    # what follows the outermost object is not looked at; a deeper array around nothing
    out.append(ScanCase("trailing", body([text_of(1, k) for k in range(5)]) + ' "unterminated {', OK))
    return out


def refusal_cases():
    t = [text_of(2, seed=k).decode() for k in range(5)]
    good = body(t)
    out = []

    def add(name, b, why):
        out.append(ScanCase(name, b, why))

    for k in range(5):
        member = '"%s":"%s"' % (NAMES[k], t[k])
        assert good.count(member) == 1
        gone = good.replace(member + ",", "") if k < 4 else good.replace("," + member, "")
        add("missing-%s" % NAMES[k], gone, MISSING)
        add("null-%s" % NAMES[k], good.replace(member, '"%s":null' % NAMES[k]), NOT_STRING)
        add("twice-%s" % NAMES[k], good[:-1] + "," + member + "}", TWICE)
        add("escape-%s" % NAMES[k], good.replace(member, '"%s":"%s\\/%s"' % (NAMES[k], t[k][:8], t[k][8:])), ESCAPE)
        add("cut-in-%s" % NAMES[k], good[:good.index(member) + len(member) - 3], UNTERMINATED)
    add("number", good.replace('"%s"' % t[1], "17"), NOT_STRING)
    add("array", good.replace('"%s"' % t[2], '["%s"]' % t[2]), NOT_STRING)
    add("object", good.replace('"%s"' % t[3], '{"v":"%s"}' % t[3]), NOT_STRING)
    add("unicode-escape", good.replace(t[4], "\\u0041" + t[4][1:]), ESCAPE)
    add("escaped-quote-in-value", good.replace(t[0], t[0][:4] + '\\"' + t[0][4:]), ESCAPE)
    add("only-nested", '{"odo":%s}' % good, MISSING)
    add("cut-in-tag", good[:good.index('"value"') + 9], UNTERMINATED)
    add("cut-after-backslash", '{"tags":[{"key":"abc\\', UNTERMINATED)
    add("empty", "", NO_OBJECT)
    add("blank", " \n\t", NO_OBJECT)
    add("array-top", "[%s]" % good, NO_OBJECT)
    add("bare-members", good[1:-1], NO_OBJECT)
    add("closing-first", "}" + good, NO_OBJECT)
    add("bracket-object", "[" + good[1:-1] + "]", NO_OBJECT)
    return out


def catalogue():
    return plain_cases() + refusal_cases()


def catalogue_file(cases):
    """The catalogue as tests/cpp/bodyspans_test reads it."""
    blob = [struct.pack("<I", len(cases))]
    for c in cases:
        raw = c.body.encode("utf-8")
        starts, lens = reference_spans(c.body) if c.expect == OK else ([0] * 5, [0] * 5)
        blob.append(struct.pack("<I", len(raw)) + raw + struct.pack("<i5Q5Q", c.expect, *starts, *lens))
    return b"".join(blob)


# ---- a plain Python model of the scanner, with one planted error each ---------------------------
BUGS = ("no_escapes", "no_depth", "last_wins")


def model_scan(raw: bytes, bug=None):
    """-> (OK, starts, lens) or (refusal class, None, None), as amph::body_scan.
    Planted: no_escapes (a backslash does not take the next byte along),
    no_depth (every key counts as a member), last_wins (a member given twice
    is taken from its last occurrence)."""
    n = len(raw)

    def string_end(i):
        k = i + 1
        while k < n:
            if raw[k] == 0x5C and bug != "no_escapes":
                k += 2
                continue
            if raw[k] == 0x22:
                return k
            k += 1
        return n

    have, depth, pos, opened = {}, 0, 0, False
    while pos < n:
        c = raw[pos:pos + 1]
        if c == b'"':
            e = string_end(pos)
            if e >= n:
                return UNTERMINATED, None, None
            nxt = e + 1
            if depth == 1 or (bug == "no_depth" and depth >= 1):
                j = e + 1
                while j < n and raw[j:j + 1] in b" \t\r\n":
                    j += 1
                if raw[j:j + 1] == b":":
                    key = raw[pos + 1:e]
                    for k, name in enumerate(NAMES):
                        if key != name.encode():
                            continue
                        if k in have and bug != "last_wins":
                            return TWICE, None, None
                        v = j + 1
                        while v < n and raw[v:v + 1] in b" \t\r\n":
                            v += 1
                        if raw[v:v + 1] != b'"':
                            return NOT_STRING, None, None
                        q = raw.find(b'"', v + 1)
                        if q < 0:
                            return UNTERMINATED, None, None
                        if b"\\" in raw[v + 1:q]:
                            return ESCAPE, None, None
                        have[k] = (v + 1, q - v - 1)
                        nxt = q + 1
            pos = nxt
            continue
        if c in (b"{", b"["):
            if not opened and c != b"{":
                return NO_OBJECT, None, None
            opened = True
            depth += 1
        elif c in (b"}", b"]"):
            if depth == 0:
                return NO_OBJECT, None, None
            depth -= 1
            if depth == 0:
                break
        pos += 1
    if not opened:
        return NO_OBJECT, None, None
    if len(have) < 5:
        return MISSING, None, None
    return OK, [have[k][0] for k in range(5)], [have[k][1] for k in range(5)]
