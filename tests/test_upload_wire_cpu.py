"""The span finder of the upload hop (amphora_amd.wire.masked_input_data_span)
and the text length of the "data" array (amph_masked_input_data_chars): the
parts of the MaskedInput JSON path (MaskedInput.java:25-62) that need no GPU."""
import json

from amphora_amd import wire

SID = "80fbba1b-3da8-4b1e-8a2c-cebd65229fad"
REC = [{"value": "A" * 22 + "=="}, {"value": "B" * 22 + "=="}, {"value": "+/" * 11 + "=="}]


def _compact(obj):
    return json.dumps(obj, separators=(",", ":"), ensure_ascii=False)


def _check(body, records):
    raw = body.encode("utf-8") if isinstance(body, str) else body
    span = wire.masked_input_data_span(body)
    assert span is not None
    lb, rb, rest = span
    assert raw[lb:rb + 1] == _compact(records).encode()
    assert len(raw[lb:rb + 1]) == (37 * len(records) + 1 if records else 2)
    obj = json.loads(rest)
    assert obj["data"] == [] and obj["secretId"] == SID
    return obj


def test_span_of_a_compact_body():
    tags = [{"key": "k", "value": "v", "valueType": "STRING"}]
    for records in (REC, REC[:1], []):
        body = _compact({"secretId": SID, "data": records, "tags": tags})
        for b in (body, body.encode()):
            assert _check(b, records)["tags"] == tags
    # the member order Jackson does not write, but may read
    assert _check(_compact({"tags": tags, "data": REC, "secretId": SID}), REC)["tags"] == tags


def test_span_is_not_fooled_by_tags():
    tricky = [{"key": '"data":[', "value": 'x"data":[{"value":"]', "valueType": "STRING"},
              {"key": "data", "value": "] [ }{", "valueType": "STRING"},
              {"key": "ümlaut \\", "value": "日本語\"", "valueType": "STRING"}]  # offsets are byte offsets
    for obj in ({"secretId": SID, "data": REC, "tags": tricky}, {"tags": tricky, "secretId": SID, "data": REC},
                {"tags": tricky, "data": REC, "secretId": SID}):
        body = _compact(obj)
        span = wire.masked_input_data_span(body)
        if span is not None:  # taken: then it is the real array and the rest is the real rest
            assert _check(body, REC)["tags"] == tricky
            assert _check(body.encode("utf-8"), REC)["tags"] == tricky
    # a second '"data"' anywhere (tricky[1]'s key) sends the body to the parser;
    # without it the reference's own member order is taken, escaped look-alikes and all
    assert wire.masked_input_data_span(_compact({"secretId": SID, "data": REC, "tags": tricky})) is None
    rest = tricky[:1] + tricky[2:]
    for obj in ({"secretId": SID, "data": REC, "tags": rest}, {"tags": rest, "data": REC, "secretId": SID}):
        assert _check(_compact(obj), REC)["tags"] == rest
        assert _check(_compact(obj).encode("utf-8"), REC)["tags"] == rest


def test_other_layouts_are_left_to_the_parser():
    tags = [{"key": "k", "value": "v", "valueType": "STRING"}]
    obj = {"secretId": SID, "data": REC, "tags": tags}
    assert wire.masked_input_data_span(json.dumps(obj, indent=2)) is None  # "data" : [
    assert wire.masked_input_data_span(json.dumps(obj)) is None  # "data": [
    assert wire.masked_input_data_span(_compact({"secretId": SID, "tags": tags})) is None
    assert wire.masked_input_data_span(_compact({"secretId": SID, "data": None, "tags": tags})) is None
    # a "data" array that is not the outermost object's member
    nested = {"secretId": SID, "tags": [{"key": "k", "value": "v", "data": [1, 2]}]}
    assert wire.masked_input_data_span(_compact(nested)) is None
    both = {"secretId": SID, "data": REC, "tags": [{"key": "k", "value": "v", "data": [1]}]}
    assert wire.masked_input_data_span(_compact(both)) is None  # the key twice: the general parser's
    assert wire.masked_input_data_span('{"secretId":"x","data":[{"value":"AAAA"}') is None  # no ']'
    assert wire.masked_input_data_span('{"secretId":"x') is None


def test_a_cut_span_never_has_the_compact_length_by_accident():
    """A ']' inside a record's string ends the span early; what is cut is then
    not a whole number of records that all carry the frame, which the fused
    call checks byte by byte -- here: the span ends inside the record."""
    body = _compact({"secretId": SID, "data": [{"value": "AAAA]AAAAAAAAAAAAAAAAA=="}, REC[0]], "tags": []})
    lb, rb, _ = wire.masked_input_data_span(body)
    assert body[lb:rb + 1] == '[{"value":"AAAA]'


def test_data_text_length():
    from amphora_amd import _lib
    chars = _lib.lib.amph_masked_input_data_chars
    assert [chars(w) for w in (0, 1, 2, 128, 1 << 22)] == [2, 38, 75, 37 * 128 + 1, 37 * (1 << 22) + 1]
    assert chars(3) == len(_compact(REC))
