"""Many MaskedInput uploads per launch (include/amphora_upload_batch.h), the
parts that need no GPU:

* the tile ownership rule at the two tile sizes of the upload kernels
  (t = 128: k_conv_json_seg, t = 192: k_mask_json_seg) with empty objects,
  whose "[]" belongs to workgroup g(o), against a linear enumeration --
  through the stand-alone program tests/cpp/uploadtiles_test.cpp, plain and
  under ASan + UBSan (a host program with its own main);
* amph_upload_slot_chars;
* the extension header's own export list;
* every argument check that returns before any GPU work, on a context
  created without a GPU.
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
KEY = (12345).to_bytes(16, "little")


def data_chars(words):
    return 37 * words + 1 if words else 2


def nchars_of(words):
    return 4 * ((16 * words + 2) // 3)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def binary(request):
    import build_native
    return build_native.build_uploadtiles_test(sanitize=request.param == "sanitized")


def test_every_tile_and_every_empty_object_has_exactly_one_workgroup(binary):
    r = subprocess.run([binary], capture_output=True, text=True, timeout=600, env=_ENV)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
    m = re.search(r"uploadtiles ok \((\d+) tables\)", r.stdout)
    assert m and int(m.group(1)) > 20000, r.stdout


SLOT_WORDS = [0, 1, 2, 3, 127, 128, 129]


def test_slot_chars_of_the_program(binary):
    r = subprocess.run([binary, "slot"] + [str(w) for w in SLOT_WORDS], capture_output=True, text=True, timeout=60,
                       env=_ENV)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [tuple(map(int, line.split())) for line in r.stdout.splitlines()]
    assert rows == [(w, data_chars(w), -(-data_chars(w) // 16) * 16) for w in SLOT_WORDS]


@pytest.fixture(scope="module")
def L():
    import amphora_amd
    return amphora_amd._lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.Context(P, R, RINV)  # no HIP call until a launch


def test_slot_chars_of_the_library(L):
    for w in SLOT_WORDS:
        got = L.lib.amph_upload_slot_chars(w)
        assert got == -(-data_chars(w) // 16) * 16 and got % 16 == 0 and 0 <= got - data_chars(w) < 16, w
        assert L.lib.amph_masked_input_data_chars(w) == data_chars(w) == L.masked_input_data_chars(w)
    assert [L.lib.amph_upload_slot_chars(w) for w in SLOT_WORDS] == [16, 48, 80, 112, 4704, 4752, 4784]
    assert L.upload_slot_chars(129) == 4784


def header_functions(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(amph_[a-z0-9_]+)\s*\(", src)))


def test_the_extension_header_has_its_own_export_list(L):
    names = header_functions("amphora_upload_batch.h")
    assert names == sorted(["amph_upload_slot_chars", "amph_upload_batch_copies", "amph_convert_share_json_packed",
                            "amph_convert_share_json_batch", "amph_mask_input_json_packed",
                            "amph_mask_input_json_batch"])
    lib = C.CDLL(L.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), n
    assert sorted(L.EXPORTED_UPLOAD_BATCH) == names
    assert not set(L.EXPORTED_UPLOAD_BATCH) & (set(L.EXPORTED) | set(L.EXPORTED_WIRE_BATCH))
    assert set(L.EXPORTED) == set(header_functions("amphora.h"))
    assert set(L.EXPORTED_WIRE_BATCH) == set(header_functions("amphora_wire_batch.h"))
    for name in ("convert_share_json_packed", "convert_share_json_batch", "mask_input_json_packed",
                 "mask_input_json_batch", "upload_batch_copies"):
        assert callable(getattr(L.Context, name))
    from amphora_amd import client, service
    assert callable(client.create_masked_input_bodies)
    assert callable(service.SecretShareUtil.convert_masked_inputs_json)
    import build_native
    assert os.path.join(ROOT, "include", "amphora_upload_batch.h") in build_native.DEPS


# ---- convert side ---------------------------------------------------------------
def _conv_packed(L, ctx, woff, toff, texts_len, flags=0):
    wo, to = np.asarray(woff, np.uint64), np.asarray(toff + [0], np.uint64)
    K = len(woff) - 1
    T = max(1, int(max(woff)))
    text = np.full(max(16, texts_len), ord("["), np.uint8)
    tup, out = np.zeros((T, 32), np.uint8), np.zeros((T, 32), np.uint8)
    bad = np.full(max(1, K), 99, np.int64)
    st = L.lib.amph_convert_share_json_packed(ctx._h, text.ctypes.data, texts_len, wo.ctypes.data, to.ctypes.data, K,
                                              tup.ctypes.data, KEY, 0, out.ctypes.data, bad.ctypes.data, flags, None)
    return st, L.lib.amph_last_error().decode()


# two objects of 3 and 2 words: texts of 112 and 75 characters
@pytest.mark.parametrize("woff,toff,texts_len,word", [
    ([0, 3, 2], [0, 112], 200, "word_offsets"),       # decreasing
    ([1, 3, 5], [0, 112], 200, "word_offsets"),       # does not start at 0
    ([0, 3, 5], [0, 112], 186, "runs past"),          # the last text ends at 187
    ([0, 3, 5], [89, 0], 200, "runs past"),           # object 0 ends at 201
    ([0, 3, 5], [2 ** 64 - 8, 0], 200, "runs past"),  # the end wraps
], ids=["w-decreasing", "w-first-not-0", "t-past-end", "t-first-past-end", "t-wraps"])
def test_convert_packed_refuses_broken_host_tables(L, ctx, woff, toff, texts_len, word):
    st, msg = _conv_packed(L, ctx, woff, toff, texts_len)
    assert st == E_PARAM and word in msg, (st, msg)


def test_convert_packed_refuses_host_io_and_takes_no_objects(L, ctx):
    st, msg = _conv_packed(L, ctx, [0, 3, 5], [0, 112], 187, flags=F_HOST_IO)
    assert st == E_PARAM and "AMPH_F_HOST_IO" in msg, (st, msg)
    assert _conv_packed(L, ctx, [0], [], 0)[0] == OK
    assert _conv_packed(L, ctx, [0], [], 0, flags=F_DEVICE)[0] == OK
    assert L.lib.amph_upload_batch_copies(ctx._h) == 0


def _conv_batch(L, ctx, lens, words, flags=0):
    K = len(words)
    texts = [np.full(max(16, n), ord("["), np.uint8) for n in lens] or [np.zeros(16, np.uint8)]
    tups = [np.zeros((max(1, w), 32), np.uint8) for w in words] or [np.zeros((1, 32), np.uint8)]
    outs = [np.zeros((max(1, w), 32), np.uint8) for w in words] or [np.zeros((1, 32), np.uint8)]
    pp = lambda xs: (C.c_void_p * len(xs))(*[x.ctypes.data for x in xs])  # noqa: E731
    sz = lambda xs: (C.c_size_t * max(1, K))(*xs)  # noqa: E731
    bad = np.full(max(1, K), 99, np.int64)
    st = L.lib.amph_convert_share_json_batch(ctx._h, pp(texts), sz(lens), sz(words), K, pp(tups), KEY, 0, pp(outs),
                                             bad.ctypes.data_as(C.POINTER(C.c_int64)), flags)
    return st, L.lib.amph_last_error().decode()


@pytest.mark.parametrize("flags", [F_DEVICE, F_ACCUMULATE, F_HOST_IO])
def test_convert_gather_refuses_every_flag(L, ctx, flags):
    assert _conv_batch(L, ctx, [112, 75], [3, 2], flags=flags)[0] == E_PARAM


def test_convert_gather_names_the_object_of_a_wrong_length(L, ctx):
    st, msg = _conv_batch(L, ctx, [112, 76, 38], [3, 2, 1])
    assert st == E_LEN and "object 1" in msg and "expected 75" in msg, (st, msg)
    st, msg = _conv_batch(L, ctx, [112, 75, 2], [3, 2, 1])  # "[]" for one word
    assert st == E_LEN and "object 2" in msg and "expected 38" in msg, (st, msg)
    st, msg = _conv_batch(L, ctx, [1], [0])  # an empty object's text is "[]"
    assert st == E_LEN and "object 0" in msg and "expected 2" in msg, (st, msg)
    assert _conv_batch(L, ctx, [], [])[0] == OK


# ---- mask side --------------------------------------------------------------------
def _texts(L, n, nchars):
    bufs = [np.full((5, max(16, max(nchars))), ord("A"), np.uint8) for _ in range(n)]
    arr = (L._AmphOdoB64 * n)()
    for j in range(n):
        arr[j] = L._AmphOdoB64(*[bufs[j][k].ctypes.data for k in range(5)], nchars[j])
    return arr, bufs


def _mask_packed(L, ctx, arr, n, woff, toff, ooff, out_cap, flags=0):
    wo, to, oo = (np.asarray(x, np.uint64) for x in (woff, toff + [0], ooff + [0]))
    K = len(woff) - 1
    T = max(1, int(max(woff)))
    sec = np.zeros((T, 16), np.uint8)
    out = np.zeros(max(16, out_cap), np.uint8)
    ff, bad = np.full(max(1, K), 99, np.int64), np.full(max(1, K), 99, np.int64)
    st = L.lib.amph_mask_input_json_packed(ctx._h, arr, n, wo.ctypes.data, to.ctypes.data, K, sec.ctypes.data,
                                           out.ctypes.data, out_cap, oo.ctypes.data, ff.ctypes.data, bad.ctypes.data,
                                           flags, None)
    return st, L.lib.amph_last_error().decode(), out


# two objects of 3 and 2 words: field texts of 64 and 44 characters, "data"
# texts of 112 and 75 characters
@pytest.mark.parametrize("woff,toff,ooff,cap,word", [
    ([0, 3, 5], [0, 64], [0, 120], 256, "multiple of 16"),   # unaligned output slot
    ([0, 3, 5], [0, 64], [8, 128], 256, "multiple of 16"),
    ([0, 3, 5], [0, 64], [0, 96], 256, "next slot"),         # overlap: object 0's text ends at 112
    ([0, 3, 5], [0, 64], [112, 0], 256, "next slot"),        # out of order
    ([0, 3, 5], [0, 64], [0, 112], 186, "output capacity"),  # the last text ends at 187
    ([0, 3, 5], [0, 72], [0, 112], 256, "multiple of 16"),   # the input tables' own checks still hold
    ([0, 3, 5], [0, 48], [0, 112], 256, "next slot"),
    ([0, 3, 2], [0, 64], [0, 112], 256, "word_offsets"),
], ids=["o-unaligned", "o-unaligned-first", "o-overlap", "o-unordered", "o-past-cap", "t-unaligned", "t-overlap",
        "w-decreasing"])
def test_mask_packed_refuses_broken_host_tables(L, ctx, woff, toff, ooff, cap, word):
    arr, keep = _texts(L, 2, [128, 128])
    st, msg, out = _mask_packed(L, ctx, arr, 2, woff, toff, ooff, cap)
    assert st == E_PARAM and word in msg, (st, msg)
    assert not out.any()


def test_mask_packed_refuses_host_io_and_unequal_parties_and_writes_empty_texts(L, ctx):
    arr, keep = _texts(L, 2, [128, 128])
    st, msg, _ = _mask_packed(L, ctx, arr, 2, [0, 3, 5], [0, 64], [0, 112], 187, flags=F_HOST_IO)
    assert st == E_PARAM and "AMPH_F_HOST_IO" in msg, (st, msg)
    arr, keep = _texts(L, 2, [128, 112])
    st, msg, _ = _mask_packed(L, ctx, arr, 2, [0, 3, 5], [0, 64], [0, 112], 187)
    assert st == E_LEN and "party 1" in msg, (st, msg)
    assert _mask_packed(L, ctx, arr, 2, [0], [], [], 0)[0] == OK
    assert _mask_packed(L, ctx, arr, 2, [0], [], [], 0, flags=F_DEVICE)[0] == OK
    # all objects empty: nothing to launch, and every text is "[]" in its own slot
    arr, keep = _texts(L, 2, [0, 0])
    st, msg, out = _mask_packed(L, ctx, arr, 2, [0, 0, 0], [0, 0], [0, 16], 18)
    assert st == OK, (st, msg)
    assert out[:18].tobytes() == b"[]" + bytes(14) + b"[]"
    assert L.lib.amph_upload_batch_copies(ctx._h) == 0


def _mask_batch(L, ctx, arr, n, words, flags=0):
    K = len(words)
    secs = [np.zeros((max(1, w), 16), np.uint8) for w in words] or [np.zeros((1, 16), np.uint8)]
    outs = [np.zeros(max(16, data_chars(w)), np.uint8) for w in words] or [np.zeros(16, np.uint8)]
    pp = lambda xs: (C.c_void_p * len(xs))(*[x.ctypes.data for x in xs])  # noqa: E731
    wd = (C.c_size_t * max(1, K))(*words)
    ff, bad = np.full(max(1, K), 99, np.int64), np.full(max(1, K), 99, np.int64)
    i64p = C.POINTER(C.c_int64)
    st = L.lib.amph_mask_input_json_batch(ctx._h, arr, n, K, wd, pp(secs), pp(outs), ff.ctypes.data_as(i64p),
                                          bad.ctypes.data_as(i64p), flags)
    return st, L.lib.amph_last_error().decode(), outs, ff, bad


@pytest.mark.parametrize("flags", [F_DEVICE, F_ACCUMULATE, F_HOST_IO])
def test_mask_gather_refuses_every_flag(L, ctx, flags):
    arr, keep = _texts(L, 4, [64, 64, 44, 44])  # 2 objects x 2 parties
    assert _mask_batch(L, ctx, arr, 2, [3, 2], flags=flags)[0] == E_PARAM


def test_mask_gather_names_the_object_and_party_of_a_length_mismatch(L, ctx):
    arr, keep = _texts(L, 6, [64, 64, 44, 48, 24, 24])  # object 1, party 1: 48 characters for 2 words
    st, msg, _, _, _ = _mask_batch(L, ctx, arr, 2, [3, 2, 1])
    assert st == E_LEN and "object 1" in msg and "party 1" in msg and "expected 44" in msg, (st, msg)
    arr, keep = _texts(L, 2, [128, 128])
    assert _mask_batch(L, ctx, arr, 2, [])[0] == OK
    arr, keep = _texts(L, 4, [0, 0, 0, 0])
    st, msg, outs, ff, bad = _mask_batch(L, ctx, arr, 2, [0, 0])
    assert st == OK and list(ff) == [-1, -1] and list(bad) == [-1, -1], (st, msg)
    assert [o[:2].tobytes() for o in outs] == [b"[]", b"[]"]
