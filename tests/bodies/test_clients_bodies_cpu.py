"""The body calls of the K-secret client session (include/
amphora_client_bodies.h), the parts that need no GPU: the header's export list
against the library's dynamic symbols, the build id, the Python entry points,
the argument checks that return before any GPU work, the scanner against
wire.odo_field_texts on the catalogue of tests/bodies_cases.py (every plain
body accepted with the reference's spans, every refusal class refused by its
reason), a Python model of the scanner that equals it and with ONE planted
error each does not, the granule rule against the texts' bytes, and the
stand-alone ASan/UBSan program on the catalogue from exact-size heap buffers.
"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import bodies_cases as BC

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tools"))
_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def L():
    import amphora_amd
    return amphora_amd._lib


@pytest.fixture(scope="module")
def cases():
    return BC.catalogue()


def header_functions(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(amph_[a-z0-9_]+)\s*\(", src)))


# ---- the ABI family ------------------------------------------------------------------------------
def test_the_extension_header_has_its_own_export_list(L):
    names = header_functions("amphora_client_bodies.h")
    assert names == ["amph_bodies_party", "amph_bodies_party_dev", "amph_bodies_scan"]
    assert sorted(L.EXPORTED_CLIENT_BODIES) == names
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r"\b(amph_bodies_[a-z0-9_]+)\b", nm))) == names
    others = (set(L.EXPORTED) | set(L.EXPORTED_WIRE_BATCH) | set(L.EXPORTED_UPLOAD_BATCH) |
              set(L.EXPORTED_RESPOND_BATCH) | set(L.EXPORTED_EXCHANGE_BATCH) | set(L.EXPORTED_PARTY_BATCH) |
              set(L.EXPORTED_CLIENT_SESSION) | set(L.EXPORTED_CLIENTS_SESSION))
    assert not set(L.EXPORTED_CLIENT_BODIES) & others
    # everything the library exports is declared by one of the headers' lists
    every = set(re.findall(r"\b(amph_[a-z0-9_]+)\b", nm))
    assert every == others | set(L.EXPORTED_CLIENT_BODIES)
    # the header states its contract, who keeps which call and what is out of scope
    text = open(os.path.join(ROOT, "include", "amphora_client_bodies.h")).read()
    for word in ("WHICH BYTES ARE READ", "WHO KEEPS WHICH CALL", "OUT OF SCOPE", "one-secret session",
                 "packed whole calls", "GPU-side scanner", "JNI and C++ mirrors", "AMPH_BODY_ABSENT"):
        assert word in text, word
    assert L.AMPH_BODY_ABSENT == 2 ** 64 - 1


def test_the_build_id_covers_the_new_unit_and_headers():
    import build_native
    assert os.path.join(ROOT, "include", "amphora_client_bodies.h") in build_native.DEPS
    assert os.path.join(build_native.CSRC, "bodyspans.hpp") in build_native.DEPS
    assert os.path.join(build_native.CSRC, "clients_bodies.hip") in build_native.SOURCES
    assert not [f for f in os.listdir(build_native.CSRC) if f.startswith("capi") and "bodies" in f]
    # bodyspans.hpp compiles for the host alone: no HIP header
    hdr = open(os.path.join(build_native.CSRC, "bodyspans.hpp")).read()
    assert "hip/" not in hdr and "__global__" not in hdr


def test_the_python_entry_points_exist(L):
    from amphora_amd import client
    assert callable(L.bodies_scan) and issubclass(L.BodyNotPlain, ValueError)
    for name in ("party_bodies", "party_bodies_dev", "scan_bodies"):
        assert callable(getattr(L.ClientSessions, name))
    import inspect
    assert inspect.signature(client.ResponseSessions.__init__).parameters["in_place"].default is True
    assert list(inspect.signature(L.ClientSessions.party_bodies).parameters)[:4] == ["self", "slot", "bodies", "starts"]


def test_the_new_unit_keeps_the_host_ordering_rule():
    """One hipMemcpyAsync, host to device, whose source is the session's
    page-locked starts image; no stream-ordered allocation; blocking copies
    only through the shared BatchImage."""
    import build_native
    code = re.sub(r"//[^\n]*", "", open(os.path.join(build_native.CSRC, "clients_bodies.hip")).read())
    calls = re.findall(r"\bhipMemcpy(?:2D)?Async\s*\(([^;]*)\);", code)
    assert len(calls) == 1 and "hipMemcpyHostToDevice" in calls[0] and "p->d_starts, table" in calls[0]
    assert "p->starts_host" in code and "hipMallocAsync" not in code and "hipMemcpy(" not in code
    assert "wire_batch_status(" in code and "int wire_batch_status(" not in code


def test_argument_checks_return_before_any_gpu_work(L):
    from oracle import amphora_oracle as O
    ctx = L.Context(O.TEST_PRIME, O.TEST_R, O.TEST_RINV)  # no HIP call until a launch
    lib, E_PARAM = L.lib, L.AMPH_E_PARAM
    out = np.zeros(10, np.uint64)
    p = out.ctypes.data
    for args in ((None, 0, p, p), (b"{}", 2, None, p), (b"{}", 2, p, None)):
        assert lib.amph_bodies_scan(*args) == E_PARAM and "null body" in lib.amph_last_error().decode()
    assert lib.amph_bodies_scan(b"{}", 2, p, p + 40) == E_PARAM
    assert lib.amph_last_error().decode() == "not a plain response body: a member is missing"
    assert not out.any()  # nothing is written on a refusal
    assert lib.amph_bodies_party(None, 0, None, None, None) == E_PARAM
    assert "null client batch session" in lib.amph_last_error().decode()
    assert lib.amph_bodies_party_dev(None, 0, None, 0, None, None) == E_PARAM
    assert "null client batch session" in lib.amph_last_error().decode()
    # a misaligned device buffer is refused before the device is selected
    assert ctx.stats()["kernel_launches"] == 0
    with pytest.raises(L.BodyNotPlain, match="no enclosing object"):
        L.bodies_scan(b"")


# ---- the scanner against the reference -------------------------------------------------------------
def test_the_catalogue_covers_what_it_claims(cases):
    plain = [c for c in cases if c.expect == BC.OK]
    names = " ".join(c.name for c in plain)
    for W in range(4):
        for form in ("compact", "pretty"):
            for r in range(5):
                assert "W%d-%s-rot%d-" % (W, form, r) in names
    for tags in BC.TAGS:
        assert "-%s-" % tags in names
    assert '\\"' in BC.TAGS["quotes"] and '\\\\\\"' in BC.TAGS["quotes"] and "rShares" in BC.TAGS["names"]
    assert any(ord(ch) > 127 for ch in BC.TAGS["unicode"]) and "}{][" in BC.TAGS["braces"]
    assert {c.expect for c in cases} == set(range(7))  # every refusal class occurs
    assert len({c.name for c in cases}) == len(cases)


def test_every_plain_body_is_accepted_with_the_references_spans(L, cases):
    from amphora_amd import wire
    n = 0
    for c in cases:
        if c.expect != BC.OK:
            continue
        raw = c.body.encode("utf-8")
        starts, lens = L.bodies_scan(raw)  # raises if the scanner refuses: it may refuse none of them
        want = BC.reference_spans(c.body)
        assert ([int(x) for x in starts], [int(x) for x in lens]) == want, c.name
        vals = wire.odo_field_texts(c.body)[0]
        assert [raw[int(a):int(a) + int(m)].decode() for a, m in zip(starts, lens)] == vals, c.name
        n += 1
    assert n >= 4 * 2 * 5 * len(BC.TAGS)


def test_every_refusal_class_is_refused_by_its_reason(L, cases):
    seen = set()
    for c in cases:
        if c.expect == BC.OK:
            continue
        with pytest.raises(L.BodyNotPlain) as e:
            L.bodies_scan(c.body.encode("utf-8"))
        assert str(e.value) == "not a plain response body: " + BC.REASONS[c.expect], (c.name, str(e.value))
        seen.add(c.expect)
    assert seen == set(BC.REASONS)


def test_the_model_equals_the_scanner_and_each_planted_error_does_not(L, cases):
    def native(raw):
        try:
            s, n = L.bodies_scan(raw)
            return BC.OK, [int(x) for x in s], [int(x) for x in n]
        except L.BodyNotPlain as e:
            why = [k for k, v in BC.REASONS.items() if str(e).endswith(": " + v)]
            return why[0], None, None
    got = {c.name: native(c.body.encode("utf-8")) for c in cases}
    for c in cases:
        assert BC.model_scan(c.body.encode("utf-8")) == got[c.name], c.name
        assert got[c.name][0] == c.expect, c.name
    for bug in BC.BUGS:
        off = [c.name for c in cases if BC.model_scan(c.body.encode("utf-8"), bug) != got[c.name]]
        assert off, "no case of the catalogue sees the planted error %s" % bug
    # each error is seen where it should be: escapes in the tags, nested names, the duplicates
    assert any("quotes" in n for n in [c.name for c in cases
                                       if BC.model_scan(c.body.encode(), "no_escapes") != got[c.name]])
    assert any("nested" in n for n in [c.name for c in cases
                                       if BC.model_scan(c.body.encode(), "no_depth") != got[c.name]])
    assert all(n.startswith("twice-") for n in [c.name for c in cases
                                                if BC.model_scan(c.body.encode(), "last_wins") != got[c.name]])


# ---- the stand-alone program ---------------------------------------------------------------------
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def binary(request):
    import build_native
    return build_native.build_bodyspans_test(sanitize=request.param == "sanitized")


def test_the_catalogue_from_exact_size_heap_buffers_is_clean(binary, cases, tmp_path):
    """Its own main, -fsanitize=address,undefined in the sanitized build: every
    body and every prefix of it scanned from a heap buffer of exactly its
    length; the spans are the reference's."""
    path = tmp_path / "catalogue.bin"
    path.write_bytes(BC.catalogue_file(cases))
    r = subprocess.run([binary, str(path)], capture_output=True, text=True, timeout=600, env=_ENV)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
    assert out.startswith("clean: ") and "%d catalogue bodies" % len(cases) in out
    if os.sep + "sanitize" + os.sep in binary:
        import build_native
        assert "-fsanitize=address" in build_native.SAN_FLAGS and "-fsanitize=undefined" in build_native.SAN_FLAGS
        nm = subprocess.run(["nm", binary], capture_output=True, text=True).stdout
        assert "__asan_init" in nm


def test_the_granule_rule_names_exactly_the_granules_that_hold_text(binary):
    pairs = [(4096 + 48 + residue, nchars) for residue in range(16) for around in (16, 4096, 8192)
             for nchars in (around - 4, around - 1, around, around + 1, around + 4, around + 15, around + 16)]
    r = subprocess.run([binary, "granules"] + [str(x) for p in pairs for x in p], capture_output=True, text=True,
                       timeout=120, env=_ENV)
    assert r.returncode == 0, r.stderr
    blocks = r.stdout.split("# ")[1:]
    assert len(blocks) == len(pairs)
    for (start, nchars), block in zip(pairs, blocks):
        rows = [[int(x) for x in line.split()] for line in block.split("\n") if line]
        residue = start & 15
        assert rows[0][:2] == [start, nchars]
        want = sorted({(start + i) >> 4 for i in range(nchars)})
        assert list(range(rows[0][2], rows[0][3])) == want, (residue, nchars)
        named = set()
        for u, (first, n, res) in enumerate(rows[1:]):
            mine = sorted({(start + i) >> 4 for i in range(16 * u, min(16 * u + 16, nchars))})
            assert list(range(first, first + n)) == mine and res == residue, (residue, nchars, u)
            if 16 * u + 16 <= nchars:  # a whole unit: two granules unless the text starts on one
                assert n == (2 if residue else 1)
            named |= set(mine)
        assert sorted(named) == want
