"""Many Output Delivery responses' base64 fields per launch
(include/amphora_respond_batch.h), the parts that need no GPU:

* the tile geometry of k_odo_b64_seg (amphora_amd/csrc/respondtiles.hpp)
  against a linear enumeration, and under hostile tables -- through the
  stand-alone program tests/cpp/respondtiles_test.cpp, plain and under
  ASan + UBSan (a host program with its own main, nothing preloaded);
* the extension header's own export list;
* every argument check that returns before any GPU work, on a context
  created without a GPU.

BROKEN_DEVICE_TABLES are the tables tests/test_respond_batch.py hands the
device call; they pass the program's bounds check here first.
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

# (T, nchars, word_offsets[K + 1], text_offsets[K]) that break the contract
BROKEN_DEVICE_TABLES = {
    "decreasing": (300, 8192, [0, 200, 100, 260, 300], [0, 4288, 4288, 6432]),
    "above-T": (300, 8192, [0, 100, 5000, 290, 300], [0, 2144, 2144, 8000]),
    "near-2^64": (300, 8192, [0, 2 ** 64 - 100, 150, 2 ** 63, 300], [2 ** 64 - 4096, 0, 2 ** 64 - 16, 4096]),
    "texts-past-nchars": (600, 4112, [0, 193, 386, 600, 600], [0, 4096, 8192, 2 ** 40]),
    "unaligned-slots": (600, 16000, [0, 193, 386, 600, 600], [3, 4127, 8255, 1]),
}


def nchars_of(words):
    return 4 * ((16 * words + 2) // 3)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def binary(request):
    import build_native
    return build_native.build_respondtiles_test(sanitize=request.param == "sanitized")


def _clean(r):
    out = r.stdout + r.stderr
    return "ERROR: AddressSanitizer" not in out and "runtime error" not in out


def test_every_character_has_one_tile_and_hostile_tables_stay_inside(binary):
    r = subprocess.run([binary], capture_output=True, text=True, timeout=600, env=_ENV)
    assert r.returncode == 0 and _clean(r), (r.stdout + r.stderr)[-4000:]
    m = re.search(r"respondtiles ok \((\d+) tables, (\d+) hostile\)", r.stdout)
    assert m and int(m.group(1)) > 3000 and int(m.group(2)) >= 8000, r.stdout


@pytest.mark.parametrize("name", sorted(BROKEN_DEVICE_TABLES))
def test_the_gpu_suites_broken_tables_stay_inside(binary, name):
    T, nchars, woff, toff = BROKEN_DEVICE_TABLES[name]
    args = [str(x) for x in [T, nchars, len(toff)] + woff + toff]
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
    names = header_functions("amphora_respond_batch.h")
    assert names == sorted(["amph_odo_fields_b64_packed", "amph_odo_fields_b64_batch", "amph_respond_batch_copies"])
    lib = C.CDLL(L.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), n
    assert sorted(L.EXPORTED_RESPOND_BATCH) == names
    assert not set(L.EXPORTED_RESPOND_BATCH) & (set(L.EXPORTED) | set(L.EXPORTED_WIRE_BATCH) |
                                                set(L.EXPORTED_UPLOAD_BATCH))
    assert set(L.EXPORTED) == set(header_functions("amphora.h"))
    for name in ("odo_fields_b64_packed", "odo_fields_b64_batch", "respond_batch_copies"):
        assert callable(getattr(L.Context, name))
    from amphora_amd import service, wire
    assert callable(wire.vss_bodies_to_json) and callable(wire.odo_bodies_to_json)
    assert callable(service.OutputDeliveryService.compute_output_delivery_objects)
    assert callable(service.OutputDeliveryService.get_input_masks_as_output_delivery_objects)
    import build_native
    assert os.path.join(ROOT, "include", "amphora_respond_batch.h") in build_native.DEPS
    assert os.path.join(build_native.CSRC, "respondtiles.hpp") in build_native.DEPS


def _packed(L, ctx, woff, toff, nchars, nbytes=None, flags=0, reject=None, fill=0x55):
    wo, to = np.asarray(woff, np.uint64), np.asarray(toff + [0], np.uint64)
    K = len(woff) - 1
    nbytes = 16 * int(woff[-1]) if nbytes is None else nbytes
    f = [np.zeros((nbytes // 16 + 1, 16), np.uint8) for _ in range(5)]
    outs = [np.full(max(16, nchars), fill, np.uint8) for _ in range(5)]
    odo = L._AmphOdo(*[x.ctypes.data for x in f], nbytes)
    ob = L._AmphOdoB64Out(*[x.ctypes.data for x in outs], nchars)
    rj = None if reject is None else np.asarray(reject, np.int64)
    st = L.lib.amph_odo_fields_b64_packed(ctx._h, C.byref(odo), wo.ctypes.data, to.ctypes.data, K, C.byref(ob),
                                          None if rj is None else rj.ctypes.data, flags, None)
    assert all((o == fill).all() for o in outs)  # refused, or nothing to write: no byte of the buffers changed
    return st, L.lib.amph_last_error().decode()


# two objects of 3 and 2 words: texts of 64 and 44 characters
@pytest.mark.parametrize("woff,toff,nchars,word", [
    ([0, 3, 2], [0, 64], 128, "word_offsets"),            # decreasing
    ([1, 3, 5], [0, 64], 128, "word_offsets"),            # does not start at 0
    ([0, 3, 5], [0, 72], 128, "multiple of 16"),          # an unaligned slot
    ([0, 3, 5], [8, 80], 128, "multiple of 16"),
    ([0, 3, 5], [0, 48], 128, "next slot"),               # overlap: object 0's text ends at 64
    ([0, 3, 5], [64, 0], 128, "next slot"),               # misordered
    ([0, 3, 5], [0, 64], 107, "buffers'"),                # the last text ends at 108
    ([0, 3, 5], [0, 2 ** 64 - 16], 128, "runs past"),     # the end wraps
], ids=["w-decreasing", "w-first-not-0", "t-unaligned", "t-unaligned-first", "t-overlap", "t-unordered",
        "t-past-nchars", "t-wraps"])
def test_packed_refuses_broken_host_tables(L, ctx, woff, toff, nchars, word):
    st, msg = _packed(L, ctx, woff, toff, nchars, nbytes=80)
    assert st == E_PARAM and word in msg, (st, msg)


def test_packed_refuses_a_table_that_does_not_end_at_t(L, ctx):
    st, msg = _packed(L, ctx, [0, 3, 5], [0, 64], 128, nbytes=96)
    assert st == E_PARAM and "differs from the fields' 6 words" in msg, (st, msg)
    st, msg = _packed(L, ctx, [0, 3, 5], [0, 64], 128, nbytes=64)
    assert st == E_PARAM and "differs from the fields' 4 words" in msg, (st, msg)


def test_packed_refuses_nbytes_that_is_no_whole_number_of_words(L, ctx):
    for nbytes in (81, 88, 95):
        st, msg = _packed(L, ctx, [0, 3, 5], [0, 64], 128, nbytes=nbytes)
        assert st == E_LEN and "multiple of 16" in msg, (st, msg)
    st, msg = _packed(L, ctx, [0, 3, 5], [0, 64], 128, nbytes=81, flags=F_DEVICE)
    assert st == E_LEN, (st, msg)


@pytest.mark.parametrize("flags", [F_ACCUMULATE, F_HOST_IO, F_DEVICE | F_ACCUMULATE, F_DEVICE | F_HOST_IO])
def test_packed_refuses_accumulate_and_host_io(L, ctx, flags):
    st, msg = _packed(L, ctx, [0, 3, 5], [0, 64], 128, flags=flags)
    assert st == E_PARAM and ("AMPH_F_ACCUMULATE" in msg or "AMPH_F_HOST_IO" in msg), (st, msg)


def test_packed_device_mode_refuses_misaligned_pointers(L, ctx):
    wo, to = np.zeros(4, np.uint64), np.zeros(4, np.uint64)
    wo[:3] = [0, 3, 5]
    to[:2] = [0, 64]
    buf = np.zeros(4096, np.uint8)
    base = buf.ctypes.data + (-buf.ctypes.data % 16)

    def call(f_at=0, o_at=0, w_at=0, r_at=None):
        odo = L._AmphOdo(*[base + 128 * k + (f_at if k == 3 else 0) for k in range(5)], 80)
        ob = L._AmphOdoB64Out(*[base + 1024 + 128 * k + (o_at if k == 1 else 0) for k in range(5)], 128)
        rj = None if r_at is None else base + 2048 + r_at
        return L.lib.amph_odo_fields_b64_packed(ctx._h, C.byref(odo), wo.ctypes.data + w_at, to.ctypes.data, 2,
                                                C.byref(ob), rj, F_DEVICE, None)
    assert call(f_at=8) == E_PARAM and call(o_at=4) == E_PARAM
    assert call(w_at=4) == E_PARAM and "8-byte aligned" in L.lib.amph_last_error().decode()
    assert call(r_at=4) == E_PARAM and "8-byte aligned" in L.lib.amph_last_error().decode()


def test_packed_takes_no_objects_and_no_words(L, ctx):
    for flags in (0, F_DEVICE):
        assert _packed(L, ctx, [0], [], 0, flags=flags)[0] == OK
        assert _packed(L, ctx, [0, 0, 0], [0, 0], 64, flags=flags)[0] == OK  # T == 0: nothing launched
    st, msg = _packed(L, ctx, [0, 0, 0], [0, 0], 64, reject=[0, -1])  # a rejected empty text stays empty
    assert st == OK, msg
    assert L.lib.amph_respond_batch_copies(ctx._h) == 0
    assert ctx.respond_batch_copies() == 0 and ctx.stats()["kernel_launches"] == 0


def _batch(L, ctx, nbytes, flags=0, reject=None):
    K = len(nbytes)
    f = [np.zeros(max(16, n + 16), np.uint8) for n in nbytes] or [np.zeros(16, np.uint8)]
    arr = (L._AmphOdo * max(1, K))()
    for o in range(K):
        arr[o] = L._AmphOdo(*[f[o].ctypes.data] * 5, nbytes[o])
    outs = [np.full(max(16, nchars_of(n // 16)), 0x55, np.uint8) for n in nbytes for _ in range(5)] or \
        [np.zeros(16, np.uint8)]
    po = (C.c_void_p * max(1, 5 * K))(*[x.ctypes.data for x in outs])
    rj = None if reject is None else np.asarray(reject, np.int64)
    st = L.lib.amph_odo_fields_b64_batch(ctx._h, arr, K, po, None if rj is None else rj.ctypes.data, flags)
    assert all((o == 0x55).all() or not o.any() for o in outs)
    return st, L.lib.amph_last_error().decode()


@pytest.mark.parametrize("flags", [F_DEVICE, F_ACCUMULATE, F_HOST_IO])
def test_gather_refuses_every_flag(L, ctx, flags):
    assert _batch(L, ctx, [48, 32], flags=flags)[0] == E_PARAM


def test_gather_names_the_object_of_a_wrong_length(L, ctx):
    st, msg = _batch(L, ctx, [48, 32, 40, 16])
    assert st == E_LEN and "object 2" in msg and "40 bytes" in msg, (st, msg)
    st, msg = _batch(L, ctx, [47])
    assert st == E_LEN and "object 0" in msg, (st, msg)
    assert _batch(L, ctx, [])[0] == OK
    assert _batch(L, ctx, [0, 0], reject=[-1, 3])[0] == OK  # no words at all: nothing launched
    assert ctx.respond_batch_copies() == 0


def test_python_wrapper_passes_the_refusals_on(L, ctx):
    f = [np.zeros((5, 16), np.uint8) for _ in range(5)]
    with pytest.raises(L.AmphoraNativeError, match="word_offsets"):
        ctx.odo_fields_b64_packed(f, [0, 3, 2])
    with pytest.raises(L.AmphoraNativeError, match="next slot"):
        ctx.odo_fields_b64_packed(f, [0, 3, 5], [0, 48], out=[np.zeros(128, np.uint8) for _ in range(5)])
    with pytest.raises(L.AmphoraNativeError, match="same length"):
        ctx.odo_fields_b64_packed(f[:4] + [np.zeros((4, 16), np.uint8)], [0, 3, 5])
    with pytest.raises(L.AmphoraNativeError, match="object 1"):
        ctx.odo_fields_b64_batch([f, [np.zeros(40, np.uint8)] * 5])
    assert ctx.odo_fields_b64_batch([]) == []
