"""Many secrets straight from their base64 wire texts
(include/amphora_wire_batch.h), the parts that need no GPU:

* the tile ownership rule of the segmented wire kernels
  (amphora_amd/csrc/wiretiles.hpp) against a linear enumeration, through the
  stand-alone program tests/cpp/wiretiles_test.cpp -- plain, and the same
  program under ASan + UBSan (the lookup's table is an exact-size array
  without entry n_objects, so a read of it is caught);
* amph_wire_slot_chars;
* the argument checks that return before any GPU work, on a context created
  without a GPU;
* the extension header's own export list.
"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle import amphora_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
P, R, RINV = O.TEST_PRIME, O.TEST_R, O.TEST_RINV
OK, E_LEN, E_PARAM = 0, 2, 3
F_DEVICE, F_ACCUMULATE, F_HOST_IO = 1, 2, 4
_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def binary(request):
    import build_native
    return build_native.build_wiretiles_test(sanitize=request.param == "sanitized")


def test_every_tile_has_exactly_one_owner(binary):
    r = subprocess.run([binary], capture_output=True, text=True, timeout=600, env=_ENV)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
    m = re.search(r"wiretiles ok \((\d+) tables\)", r.stdout)
    assert m and int(m.group(1)) > 20000, r.stdout


def nchars_of(words):
    return 4 * ((16 * words + 2) // 3)


SLOT_WORDS = [0, 1, 2, 3, 4, 5, 6, 7, 191, 192, 193]


def test_slot_chars_of_the_program(binary):
    r = subprocess.run([binary, "slot"] + [str(w) for w in SLOT_WORDS], capture_output=True, text=True, timeout=60,
                       env=_ENV)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [tuple(map(int, line.split())) for line in r.stdout.splitlines()]
    assert rows == [(w, nchars_of(w), -(-nchars_of(w) // 16) * 16) for w in SLOT_WORDS]


@pytest.fixture(scope="module")
def L():
    import amphora_amd
    return amphora_amd._lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.Context(P, R, RINV)  # no HIP call until a launch


def test_slot_chars_of_the_library(L):
    for w in SLOT_WORDS:
        got = L.lib.amph_wire_slot_chars(w)
        assert got == -(-nchars_of(w) // 16) * 16 and got % 16 == 0 and 0 <= got - nchars_of(w) < 16, w
    assert [L.lib.amph_wire_slot_chars(w) for w in (0, 1, 2, 3)] == [0, 32, 48, 64]
    assert L.wire_slot_chars(192) == 4096 and L.wire_text_chars(193) == 4120


def header_functions(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(amph_[a-z0-9_]+)\s*\(", src)))


def test_the_extension_header_has_its_own_export_list(L):
    names = header_functions("amphora_wire_batch.h")
    assert {"amph_wire_slot_chars", "amph_recombine_verify_b64_packed", "amph_mask_input_b64_packed",
            "amph_recombine_verify_b64_batch", "amph_mask_input_b64_batch"} <= set(names)
    lib = C.CDLL(L.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), n
    assert sorted(L.EXPORTED_WIRE_BATCH) == names
    assert not set(L.EXPORTED_WIRE_BATCH) & set(L.EXPORTED)
    assert set(L.EXPORTED) == set(header_functions("amphora.h"))  # the base header's list is its own
    for name in ("recombine_verify_b64_packed", "mask_input_b64_packed", "recombine_verify_b64_batch",
                 "mask_input_b64_batch"):
        assert callable(getattr(L.Context, name))
    from amphora_amd import client
    assert callable(client.verify_vss_json_batch) and callable(client.create_masked_inputs_from_bodies)


def _texts(L, n, nchars):
    """n parties' amph_odo_b64 structs over 'A' texts (never read here)."""
    bufs = [np.full((5, max(16, max(nchars))), ord("A"), np.uint8) for _ in range(n)]
    arr = (L._AmphOdoB64 * n)()
    for j in range(n):
        arr[j] = L._AmphOdoB64(*[bufs[j][k].ctypes.data for k in range(5)], nchars[j])
    return arr, bufs


def _packed(L, ctx, arr, n, woff, toff, flags=0, masked=False):
    wo, to = np.asarray(woff, np.uint64), np.asarray(toff + [0], np.uint64)
    K = len(woff) - 1
    T = max(1, int(max(woff)))
    out, sec, rec = np.zeros((T, 16), np.uint8), np.zeros((T, 16), np.uint8), np.zeros((T, 24), np.uint8)
    ff, bad = np.full(max(1, K), 99, np.int64), np.full(max(1, K), 99, np.int64)
    if masked:
        st = L.lib.amph_mask_input_b64_packed(ctx._h, arr, n, wo.ctypes.data, to.ctypes.data, K, sec.ctypes.data,
                                              out.ctypes.data, rec.ctypes.data, ff.ctypes.data, bad.ctypes.data,
                                              flags, None)
    else:
        st = L.lib.amph_recombine_verify_b64_packed(ctx._h, arr, n, wo.ctypes.data, to.ctypes.data, K,
                                                    out.ctypes.data, ff.ctypes.data, bad.ctypes.data, flags, None)
    return st, L.lib.amph_last_error().decode()


# two objects of 3 and 2 words: texts of 64 and 44 characters
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("woff,toff,nchars,word", [
    ([0, 3, 5], [0, 72], 128, "multiple of 16"),       # not a multiple of 16
    ([0, 3, 5], [8, 64], 128, "multiple of 16"),
    ([0, 3, 5], [0, 48], 128, "next slot"),            # overlap: object 0 ends at 64
    ([0, 3, 5], [64, 0], 128, "next slot"),            # out of order
    ([0, 3, 5], [0, 64], 107, "buffers'"),             # the last text ends at 108
    ([0, 3, 5], [0, 96], 128, "buffers'"),
    ([0, 3, 2], [0, 64], 128, "word_offsets"),         # decreasing
    ([1, 3, 5], [0, 64], 128, "word_offsets"),         # does not start at 0
], ids=["t-unaligned", "t-unaligned-first", "t-overlap", "t-unordered", "t-past-end", "t-slot-past-end",
        "w-decreasing", "w-first-not-0"])
def test_packed_refuses_broken_host_tables(L, ctx, masked, woff, toff, nchars, word):
    arr, keep = _texts(L, 2, [nchars, nchars])
    st, msg = _packed(L, ctx, arr, 2, woff, toff, masked=masked)
    assert st == E_PARAM and word in msg, (st, msg)


@pytest.mark.parametrize("masked", [False, True])
def test_packed_accepts_the_exact_fit_and_refuses_host_io_and_unequal_parties(L, ctx, masked):
    arr, keep = _texts(L, 2, [128, 128])
    st, msg = _packed(L, ctx, arr, 2, [0, 3, 5], [0, 64], flags=F_HOST_IO, masked=masked)
    assert st == E_PARAM and "AMPH_F_HOST_IO" in msg, (st, msg)
    arr, keep = _texts(L, 2, [128, 112])
    st, msg = _packed(L, ctx, arr, 2, [0, 3, 5], [0, 64], masked=masked)
    assert st == E_LEN and "party 1" in msg, (st, msg)
    # all objects empty: valid tables, nothing to launch, every verdict clean
    arr, keep = _texts(L, 2, [0, 0])
    st, msg = _packed(L, ctx, arr, 2, [0, 0, 0], [0, 0], masked=masked)
    assert st == OK, (st, msg)


def _batch(L, ctx, arr, n, words, flags=0, masked=False):
    K = len(words)
    W = max([1] + list(words))
    mk = lambda width: [np.zeros((W, width), np.uint8) for _ in range(max(1, K))]  # noqa: E731
    pp = lambda xs: (C.c_void_p * max(1, K))(*[x.ctypes.data for x in xs])  # noqa: E731
    outs, secs, recs = mk(16), mk(16), mk(24)
    wd = (C.c_size_t * max(1, K))(*words)
    ff, bad = np.full(max(1, K), 99, np.int64), np.full(max(1, K), 99, np.int64)
    i64p = C.POINTER(C.c_int64)
    if masked:
        st = L.lib.amph_mask_input_b64_batch(ctx._h, arr, n, K, wd, pp(secs), pp(outs), pp(recs),
                                             ff.ctypes.data_as(i64p), bad.ctypes.data_as(i64p), flags)
    else:
        st = L.lib.amph_recombine_verify_b64_batch(ctx._h, arr, n, K, wd, pp(outs), ff.ctypes.data_as(i64p),
                                                   bad.ctypes.data_as(i64p), flags)
    return st, L.lib.amph_last_error().decode(), ff, bad


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("flags", [F_DEVICE, F_ACCUMULATE, F_HOST_IO])
def test_gather_refuses_every_flag(L, ctx, masked, flags):
    arr, keep = _texts(L, 4, [64, 64, 44, 44])  # 2 objects x 2 parties
    assert _batch(L, ctx, arr, 2, [3, 2], flags=flags, masked=masked)[0] == E_PARAM


@pytest.mark.parametrize("masked", [False, True])
def test_gather_names_the_object_and_party_of_a_length_mismatch(L, ctx, masked):
    arr, keep = _texts(L, 6, [64, 64, 44, 48, 24, 24])  # object 1, party 1: 48 characters for 2 words
    st, msg, _, _ = _batch(L, ctx, arr, 2, [3, 2, 1], masked=masked)
    assert st == E_LEN and "object 1" in msg and "party 1" in msg and "expected 44" in msg, (st, msg)
    arr, keep = _texts(L, 6, [64, 64, 44, 44, 24, 24])
    st, msg, _, _ = _batch(L, ctx, arr, 2, [3, 2, 2], masked=masked)
    assert st == E_LEN and "object 2" in msg and "party 0" in msg, (st, msg)


@pytest.mark.parametrize("masked", [False, True])
def test_no_objects_and_empty_objects_launch_nothing(L, ctx, masked):
    arr, keep = _texts(L, 2, [128, 128])
    assert _packed(L, ctx, arr, 2, [0], [], masked=masked)[0] == OK
    assert _packed(L, ctx, arr, 2, [0], [], flags=F_DEVICE, masked=masked)[0] == OK
    assert _batch(L, ctx, arr, 2, [], masked=masked)[0] == OK
    arr, keep = _texts(L, 4, [0, 0, 0, 0])
    st, msg, ff, bad = _batch(L, ctx, arr, 2, [0, 0], masked=masked)
    assert st == OK and list(ff) == [-1, -1] and list(bad) == [-1, -1], (st, msg)
    assert L.lib.amph_wire_batch_copies(ctx._h) == 0
