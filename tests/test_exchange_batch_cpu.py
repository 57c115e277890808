"""Many requests' Beaver exchange texts per call
(include/amphora_exchange_batch.h), the parts that need no GPU:

* the encode's tile ownership and the decode's span ownership
  (amphora_amd/csrc/exchangetiles.hpp) against a linear enumeration, and
  under hostile tables -- through the stand-alone program
  tests/cpp/exchangetiles_test.cpp, plain and under ASan + UBSan (a host
  program with its own main, nothing preloaded);
* the extension header's own export list and constant;
* every argument check that returns before any GPU work, on a context
  created without a GPU.

BROKEN_DEVICE_TABLES are the tables tests/test_exchange_batch.py hands the
device calls; they pass the program's bounds check here first.
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
SPAN = 8192
_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

# (npairs_total, texts_len = out_cap, pair_offsets[K + 1], text_offsets[K], text_lens[K]) that break the contract
BROKEN_DEVICE_TABLES = {
    "decreasing-pairs": (600, 65536, [0, 300, 100, 500, 600], [0, 16384, 32768, 49152], [100, 100, 100, 100]),
    "past-capacity": (600, 40000, [0, 100, 200, 300, 600], [0, 8192, 2 ** 40, 2 ** 64 - 8192], [8000, 9000, 50, 50]),
    "lens-over-slot": (600, 65536, [0, 100, 200, 300, 600], [0, 8192, 16384, 24576],
                       [30000, 2 ** 63, 70000, 8192 * 5]),
    "unaligned-offset": (600, 65536, [0, 100, 200, 300, 600], [3, 8200, 16385, 40001], [100, 100, 100, 100]),
}


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def binary(request):
    import build_native
    return build_native.build_exchangetiles_test(sanitize=request.param == "sanitized")


def _clean(r):
    out = r.stdout + r.stderr
    return "ERROR: AddressSanitizer" not in out and "runtime error" not in out


def test_every_pair_and_span_has_one_owner_and_hostile_tables_stay_inside(binary):
    r = subprocess.run([binary], capture_output=True, text=True, timeout=600, env=_ENV)
    assert r.returncode == 0 and _clean(r), (r.stdout + r.stderr)[-4000:]
    m = re.search(r"exchangetiles ok \((\d+) tables, (\d+) hostile\)", r.stdout)
    assert m and int(m.group(1)) > 3000 and int(m.group(2)) >= 8000, r.stdout


@pytest.mark.parametrize("name", sorted(BROKEN_DEVICE_TABLES))
def test_the_gpu_suites_broken_tables_stay_inside(binary, name):
    npairs, nchars, poff, toff, lens = BROKEN_DEVICE_TABLES[name]
    args = [str(x) for x in [npairs, nchars, len(toff)] + poff + toff + lens]
    r = subprocess.run([binary, "tables"] + args, capture_output=True, text=True, timeout=60, env=_ENV)
    assert r.returncode == 0 and _clean(r) and r.stdout.strip() == "inside", r.stdout + r.stderr


@pytest.fixture(scope="module")
def L():
    import amphora_amd
    return amphora_amd._lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.Context(P, R, RINV)  # no HIP call until a launch


def header_functions(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(amph_[a-z0-9_]+)\s*\(", src)))


def test_the_extension_header_has_its_own_export_list(L):
    names = header_functions("amphora_exchange_batch.h")
    assert names == sorted(["amph_exchange_slot_chars", "amph_exchange_encode_packed", "amph_exchange_encode_batch",
                            "amph_exchange_decode_packed", "amph_exchange_decode_batch",
                            "amph_exchange_batch_copies"])
    lib = C.CDLL(L.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), n
    assert sorted(L.EXPORTED_EXCHANGE_BATCH) == names
    assert not set(L.EXPORTED_EXCHANGE_BATCH) & (set(L.EXPORTED) | set(L.EXPORTED_WIRE_BATCH) |
                                                 set(L.EXPORTED_UPLOAD_BATCH) | set(L.EXPORTED_RESPOND_BATCH))
    assert set(L.EXPORTED) == set(header_functions("amphora.h"))
    for name in ("exchange_encode_packed", "exchange_encode_batch", "exchange_decode_packed",
                 "exchange_decode_batch", "exchange_batch_copies"):
        assert callable(getattr(L.Context, name))
    src = open(os.path.join(ROOT, "include", "amphora_exchange_batch.h")).read()
    assert re.search(r"#define\s+AMPH_EXCHANGE_SLOT_ALIGN\s+8192\b", src) and L.AMPH_EXCHANGE_SLOT_ALIGN == SPAN
    import build_native
    assert os.path.join(ROOT, "include", "amphora_exchange_batch.h") in build_native.DEPS
    assert os.path.join(build_native.CSRC, "exchangetiles.hpp") in build_native.DEPS


def test_slot_chars_is_the_longest_text_rounded_up_to_the_span(L):
    for n in [0, 1, 2, 88, 89, 90, 255, 256, 257, 1024, 2000, 10 ** 6]:
        s, m = L.lib.amph_exchange_slot_chars(n), L.lib.amph_exchange_max_chars(n)
        assert s % SPAN == 0 and m <= s < m + SPAN and L.exchange_slot_chars(n) == s, n
    assert L.lib.amph_exchange_slot_chars(0) == SPAN and L.lib.amph_exchange_slot_chars(89) == SPAN
    assert L.lib.amph_exchange_slot_chars(90) == 2 * SPAN  # 92 * 90 + 2 = 8282


def _enc(L, ctx, poff, toff, cap, npairs=None, flags=0, fill=0x55):
    po, to = np.asarray(poff, np.uint64), np.asarray(toff + [0], np.uint64)
    K = len(poff) - 1
    npairs = int(poff[-1]) if npairs is None else npairs
    mag, neg = np.zeros((npairs + 1, 32), np.uint8), np.zeros((npairs + 1, 2), np.uint8)
    out, lens = np.full(max(16, min(cap, 1 << 20)), fill, np.uint8), np.full(max(1, K), 77, np.uint64)
    st = L.lib.amph_exchange_encode_packed(ctx._h, mag.ctypes.data, neg.ctypes.data, npairs, po.ctypes.data,
                                           to.ctypes.data, K, out.ctypes.data, cap, lens.ctypes.data, flags, None)
    assert (out == fill).all() and (lens == 77).all()  # refused, or nothing to write: nothing changed
    return st, L.lib.amph_last_error().decode()


def _dec(L, ctx, poff, toff, lens, texts_len, npairs=None, flags=0):
    po, to = np.asarray(poff, np.uint64), np.asarray(toff + [0], np.uint64)
    tl = np.asarray(lens + [0], np.uint64)
    K = len(poff) - 1
    npairs = int(poff[-1]) if npairs is None else npairs
    text = np.full(max(16, min(texts_len, 1 << 20)), 0x20, np.uint8)
    mag, neg = np.full((npairs + 1, 32), 0x55, np.uint8), np.full((npairs + 1, 2), 0x55, np.uint8)
    bad = np.full(max(1, K), 77, np.int64)
    st = L.lib.amph_exchange_decode_packed(ctx._h, text.ctypes.data, texts_len, po.ctypes.data, to.ctypes.data,
                                           tl.ctypes.data, K, npairs, mag.ctypes.data, neg.ctypes.data,
                                           bad.ctypes.data_as(C.POINTER(C.c_int64)), flags, None)
    assert (mag == 0x55).all() and (neg == 0x55).all() and (bad == 77).all()
    return st, L.lib.amph_last_error().decode()


# two objects of 3 and 90 pairs: slots of one and two spans
@pytest.mark.parametrize("poff,toff,cap,word", [
    ([0, 3, 2], [0, SPAN], 4 * SPAN, "pair_offsets"),                  # decreasing
    ([1, 3, 93], [0, SPAN], 4 * SPAN, "pair_offsets"),                 # does not start at 0
    ([0, 3, 93], [0, SPAN + 16], 4 * SPAN, "multiple of 8192"),        # an unaligned slot
    ([0, 3, 93], [16, SPAN], 4 * SPAN, "multiple of 8192"),
    ([0, 90, 93], [0, SPAN], 4 * SPAN, "next slot"),                   # object 0 needs 8282 characters
    ([0, 3, 93], [SPAN, 0], 4 * SPAN, "next slot"),                    # misordered
    ([0, 3, 93], [0, 0], 4 * SPAN, "next slot"),                       # one slot twice
    ([0, 3, 93], [0, SPAN], SPAN + 92 * 90 + 1, "out_cap"),            # the last slot one character short
    ([0, 3, 93], [0, 2 ** 64 - SPAN], 4 * SPAN, "runs past"),          # the end wraps
], ids=["p-decreasing", "p-first-not-0", "t-unaligned", "t-unaligned-first", "t-slot-too-small", "t-unordered",
        "t-same-slot", "t-past-out-cap", "t-wraps"])
def test_encode_packed_refuses_broken_host_tables(L, ctx, poff, toff, cap, word):
    st, msg = _enc(L, ctx, poff, toff, cap, npairs=93)
    assert st == E_PARAM and word in msg, (st, msg)


def test_packed_refuses_a_pair_table_that_does_not_end_at_npairs_total(L, ctx):
    st, msg = _enc(L, ctx, [0, 3, 5], [0, SPAN], 2 * SPAN, npairs=6)
    assert st == E_PARAM and "differs from npairs_total = 6" in msg, (st, msg)
    st, msg = _dec(L, ctx, [0, 3, 5], [0, SPAN], [10, 10], 2 * SPAN, npairs=4)
    assert st == E_PARAM and "differs from npairs_total = 4" in msg, (st, msg)


@pytest.mark.parametrize("poff,toff,lens,texts_len,word", [
    ([0, 3, 2], [0, SPAN], [10, 10], 2 * SPAN, "pair_offsets"),
    ([0, 3, 5], [0, SPAN + 1], [10, 10], 3 * SPAN, "multiple of 8192"),
    ([0, 3, 5], [0, SPAN], [SPAN + 1, 10], 2 * SPAN, "next slot"),       # a text longer than its slot
    ([0, 3, 5], [0, SPAN], [10, SPAN + 1], 2 * SPAN, "texts_len"),       # the last text past the buffer
    ([0, 3, 5], [0, 0], [0, 10], 2 * SPAN, "next slot"),                 # two texts in one slot
    ([0, 3, 5], [0, SPAN], [10, 2 ** 64 - 100], 2 * SPAN, "runs past"),
], ids=["p-decreasing", "t-unaligned", "l-over-slot", "l-past-texts-len", "t-same-slot", "l-wraps"])
def test_decode_packed_refuses_broken_host_tables(L, ctx, poff, toff, lens, texts_len, word):
    st, msg = _dec(L, ctx, poff, toff, lens, texts_len, npairs=5)
    assert st == E_PARAM and word in msg, (st, msg)


@pytest.mark.parametrize("flags", [F_HOST_IO, F_DEVICE | F_HOST_IO, F_ACCUMULATE, F_DEVICE | F_ACCUMULATE])
def test_encode_packed_refuses_host_io_and_accumulate(L, ctx, flags):
    st, msg = _enc(L, ctx, [0, 3, 5], [0, SPAN], 2 * SPAN, flags=flags)
    assert st == E_PARAM and ("AMPH_F_ACCUMULATE" in msg or "AMPH_F_HOST_IO" in msg), (st, msg)


@pytest.mark.parametrize("flags", [F_HOST_IO, F_DEVICE | F_HOST_IO, F_ACCUMULATE])
def test_decode_packed_refuses_host_io_and_host_accumulate(L, ctx, flags):
    st, msg = _dec(L, ctx, [0, 3, 5], [0, SPAN], [10, 10], 2 * SPAN, flags=flags)
    assert st == E_PARAM and ("AMPH_F_ACCUMULATE" in msg or "AMPH_F_HOST_IO" in msg), (st, msg)


def test_packed_device_mode_refuses_misaligned_pointers(L, ctx):
    tab = np.zeros(16, np.uint64)
    buf = np.zeros(8192, np.uint8)
    base = buf.ctypes.data + (-buf.ctypes.data % 16)
    t = tab.ctypes.data

    def enc(m_at=0, o_at=0, p_at=0, l_at=0):
        return L.lib.amph_exchange_encode_packed(ctx._h, base + m_at, base + 1024, 5, t + p_at, t + 32, 2,
                                                 base + 2048 + o_at, 4096, t + 64 + l_at, F_DEVICE, None)

    def dec(m_at=0, x_at=0, t_at=0, b_at=0):
        return L.lib.amph_exchange_decode_packed(ctx._h, base + 2048 + x_at, 4096, t, t + 32 + t_at, t + 64, 2, 5,
                                                 base + m_at, base + 1024,
                                                 C.cast(C.c_void_p(t + 96 + b_at), C.POINTER(C.c_int64)), F_DEVICE,
                                                 None)
    assert enc(m_at=8) == E_PARAM and enc(o_at=4) == E_PARAM
    assert enc(p_at=4) == E_PARAM and "8-byte aligned" in L.lib.amph_last_error().decode()
    assert enc(l_at=4) == E_PARAM and "8-byte aligned" in L.lib.amph_last_error().decode()
    assert dec(m_at=8) == E_PARAM and dec(x_at=4) == E_PARAM
    assert dec(t_at=4) == E_PARAM and "8-byte aligned" in L.lib.amph_last_error().decode()
    assert dec(b_at=4) == E_PARAM and "8-byte aligned" in L.lib.amph_last_error().decode()


def test_calls_take_no_objects(L, ctx):
    for flags in (0, F_DEVICE):
        assert _enc(L, ctx, [0], [], 0, flags=flags)[0] == OK
        assert _dec(L, ctx, [0], [], [], 0, flags=flags)[0] == OK
    assert L.lib.amph_exchange_encode_batch(ctx._h, None, None, None, 0, None, None, None, 0) == OK
    assert L.lib.amph_exchange_decode_batch(ctx._h, None, None, None, 0, None, None, None, 0) == OK
    assert ctx.exchange_encode_batch([], []) == []
    assert ctx.exchange_decode_batch([], [])[0] == []
    assert L.lib.amph_exchange_batch_copies(ctx._h) == 0
    assert ctx.exchange_batch_copies() == 0 and ctx.stats()["kernel_launches"] == 0


@pytest.mark.parametrize("flags", [F_DEVICE, F_ACCUMULATE, F_HOST_IO])
def test_gather_refuses_every_flag(L, ctx, flags):
    one = (C.c_void_p * 1)(0)
    n = (C.c_size_t * 1)(0)
    v = np.zeros(1, np.int64)
    assert L.lib.amph_exchange_encode_batch(ctx._h, one, one, n, 1, one, n, v.ctypes.data, flags) == E_PARAM
    assert "host memory only" in L.lib.amph_last_error().decode()
    assert L.lib.amph_exchange_decode_batch(ctx._h, one, n, n, 1, one, one,
                                            v.ctypes.data_as(C.POINTER(C.c_int64)), flags) == E_PARAM
    assert "host memory only" in L.lib.amph_last_error().decode()


def test_gather_names_the_object_of_a_null_buffer(L, ctx):
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data
    st = L.lib.amph_exchange_encode_batch(ctx._h, (C.c_void_p * 2)(p, 0), (C.c_void_p * 2)(p, p),
                                          (C.c_size_t * 2)(1, 1), 2, (C.c_void_p * 2)(p, p),
                                          (C.c_size_t * 2)(64, 64), np.zeros(2, np.uint64).ctypes.data, 0)
    assert st == E_PARAM and "object 1" in L.lib.amph_last_error().decode()
    st = L.lib.amph_exchange_decode_batch(ctx._h, (C.c_void_p * 2)(p, p), (C.c_size_t * 2)(2, 2),
                                          (C.c_size_t * 2)(0, 1), 2, (C.c_void_p * 2)(0, p), (C.c_void_p * 2)(0, 0),
                                          np.zeros(2, np.int64).ctypes.data_as(C.POINTER(C.c_int64)), 0)
    assert st == E_PARAM and "object 1" in L.lib.amph_last_error().decode()


def test_python_wrapper_passes_the_refusals_on(L, ctx):
    mag, neg = np.zeros((5, 2, 16), np.uint8), np.zeros((5, 2), np.uint8)
    with pytest.raises(L.AmphoraNativeError, match="pair_offsets"):
        ctx.exchange_encode_packed(mag, neg, [0, 3, 2])
    with pytest.raises(L.AmphoraNativeError, match="multiple of 8192"):
        ctx.exchange_encode_packed(mag, neg, [0, 3, 5], [0, SPAN + 16], out=np.zeros(3 * SPAN, np.uint8))
    with pytest.raises(L.AmphoraNativeError, match="next slot"):
        ctx.exchange_decode_packed(np.zeros(2 * SPAN, np.uint8), [0, 3, 5], [0, SPAN], [SPAN + 1, 2])
    with pytest.raises(ValueError, match="one text offset"):
        ctx.exchange_decode_packed(np.zeros(2 * SPAN, np.uint8), [0, 3, 5], [0], [2, 2])
