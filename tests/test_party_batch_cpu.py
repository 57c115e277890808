"""Many requests of one party in one device-resident session
(include/amphora_party_batch.h), the parts that need no GPU:

* the open-post tile ownership and the span-form windows
  (amphora_amd/csrc/partytiles.hpp) against a linear enumeration, and under
  hostile tables -- through the stand-alone program
  tests/cpp/partytiles_test.cpp, plain and under ASan + UBSan (a host program
  with its own main, nothing preloaded);
* the extension header's own export list;
* the argument checks that return before any GPU work, on a context created
  without a GPU.  (The checks that need a session -- a host call on a device
  session and the reverse, an unfilled slot at finish, a second finish -- also
  return before any GPU work, but a session exists only where begin has run:
  tests/test_party_batch.py holds them.)
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
_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def binary(request):
    import build_native
    return build_native.build_partytiles_test(sanitize=request.param == "sanitized")


def test_every_pair_has_one_tile_every_value_its_slot_and_hostile_tables_stay_inside(binary):
    r = subprocess.run([binary], capture_output=True, text=True, timeout=600, env=_ENV)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
    m = re.search(r"partytiles ok \((\d+) tables, (\d+) windows, (\d+) hostile\)", r.stdout)
    assert m and int(m.group(1)) > 3000 and int(m.group(2)) >= 3000 and int(m.group(3)) >= 8000, r.stdout


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
    names = header_functions("amphora_party_batch.h")
    assert len(names) == 18 and all(n.startswith("amph_parties_") for n in names)
    lib = C.CDLL(L.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), n
    assert sorted(L.EXPORTED_PARTY_BATCH) == names
    assert not set(L.EXPORTED_PARTY_BATCH) & (set(L.EXPORTED) | set(L.EXPORTED_WIRE_BATCH) |
                                              set(L.EXPORTED_UPLOAD_BATCH) | set(L.EXPORTED_RESPOND_BATCH) |
                                              set(L.EXPORTED_EXCHANGE_BATCH))
    assert set(L.EXPORTED) == set(header_functions("amphora.h"))
    # the library exports nothing of this family that the header does not declare
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r"\b(amph_parties_[a-z0-9_]+)\b", nm))) == names
    for name in ("parties_begin", "parties_begin_dev"):
        assert callable(getattr(L.Context, name))
    import build_native
    assert os.path.join(ROOT, "include", "amphora_party_batch.h") in build_native.DEPS
    assert os.path.join(build_native.CSRC, "partytiles.hpp") in build_native.DEPS
    assert os.path.join(build_native.CSRC, "parties_session.hip") in build_native.SOURCES


def _begin(L, ctx, woff, K, stride=32, n=3, dev=False, null=(), T=None):
    wo = np.asarray(woff, np.uint64)
    T = int(wo[-1]) if T is None else T
    sd, mk, tr = np.zeros((T + 1, stride), np.uint8), np.zeros((2 * T + 1, 32), np.uint8), np.zeros((2 * T + 1, 96),
                                                                                                   np.uint8)
    # 16-byte aligned (device mode checks its pointers first)
    ptr = lambda a, name: None if name in null else a.ctypes.data + (-a.ctypes.data % 16)  # noqa: E731
    h = C.c_void_p(1)
    args = [ctx._h, ptr(sd, "share"), stride, ptr(mk, "masks"), ptr(tr, "triples"),
            None if "offsets" in null else wo.ctypes.data, K, n, None, None, None]
    st = L.lib.amph_parties_begin_dev(*args, None, C.byref(h)) if dev else L.lib.amph_parties_begin(*args, C.byref(h))
    assert not h.value  # refused: no session
    return st, L.lib.amph_last_error().decode()


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
def test_begin_refuses_before_any_gpu_work(L, ctx, dev):
    for kw, word in [
        (dict(woff=[0, 3, 5], K=2, null=("offsets",)), "null word_offsets"),
        (dict(woff=[0], K=0), "at least one object"),
        (dict(woff=[0, 3, 2, 5], K=3), "nondecreasing (object 1)"),
        (dict(woff=[1, 3, 5], K=2), "word_offsets[0] must be 0"),
        (dict(woff=[0, 3, 5], K=2, stride=24), "share_stride must be 16 or 32"),
        (dict(woff=[0, 3, 5], K=2, n=0), "n_parties must be in [1, 16]"),
        (dict(woff=[0, 3, 5], K=2, n=17), "n_parties must be in [1, 16]"),
        (dict(woff=[0, 3, 5], K=2, null=("share",)), "null buffer"),
        (dict(woff=[0, 3, 5], K=2, null=("triples",)), "null buffer"),
    ]:
        st, msg = _begin(L, ctx, dev=dev, **kw)
        assert st == E_PARAM and word in msg, (kw, st, msg)
    assert L.lib.amph_parties_begin(ctx._h, None, 32, None, None, None, 1, 2, None, None, None, None) == E_PARAM
    assert ctx.stats()["kernel_launches"] == 0


def test_device_begin_refuses_misaligned_buffers(L, ctx):
    wo = np.asarray([0, 2], np.uint64)
    buf = np.zeros(4096, np.uint8)
    base = buf.ctypes.data + (-buf.ctypes.data % 16)
    h = C.c_void_p()
    st = L.lib.amph_parties_begin_dev(ctx._h, base + 8, 32, base + 256, base + 512, wo.ctypes.data, 1, 2, None, None,
                                      None, None, C.byref(h))
    assert st == E_PARAM and not h.value


def test_calls_on_no_session(L):
    lib = L.lib
    v = np.zeros(4, np.uint64)
    assert lib.amph_parties_objects(None) == 0 and lib.amph_parties_words(None) == 0
    assert lib.amph_parties_text_bytes(None) == 0 and lib.amph_parties_field_chars(None) == 0
    for st in (lib.amph_parties_text_offsets(None, v.ctypes.data), lib.amph_parties_field_offsets(None, v.ctypes.data),
               lib.amph_parties_text_lens(None, v.ctypes.data), lib.amph_parties_text(None, 0, v.ctypes.data, 8),
               lib.amph_parties_partner(None, 1, v.ctypes.data, v.ctypes.data, v.ctypes.data),
               lib.amph_parties_partner_dev(None, 1, v.ctypes.data, v.ctypes.data, v.ctypes.data, None),
               lib.amph_parties_reset_partner(None, 1), lib.amph_parties_finish(None, 0, None, None),
               lib.amph_parties_finish_b64(None, 0, None, None), lib.amph_parties_finish_b64_dev(None, 0, None, None)):
        assert st == E_PARAM and "null party batch session" in lib.amph_last_error().decode()
    lib.amph_parties_free(None)


def test_python_wrapper_checks_its_arrays(L, ctx):
    z = np.zeros((5, 32), np.uint8)
    with pytest.raises(L.AmphoraNativeError, match="word_offsets must end at the 5 words"):
        ctx.parties_begin(z, 32, np.zeros((10, 32), np.uint8), np.zeros((10, 96), np.uint8), [0, 3], 2)
    with pytest.raises(L.AmphoraNativeError, match="expected 10 multiplication triples"):
        ctx.parties_begin(z, 32, np.zeros((10, 32), np.uint8), np.zeros((9, 96), np.uint8), [0, 3, 5], 2)
    with pytest.raises(L.AmphoraNativeError, match="nondecreasing"):
        ctx.parties_begin(z, 32, np.zeros((10, 32), np.uint8), np.zeros((10, 96), np.uint8), [0, 6, 5], 2)


def test_the_sessions_async_copies_keep_the_host_ordering_rule():
    """The host-copy ordering rule (tests/test_host_ordering.py states it for
    the capi_* units) in this family's unit: a hipMemcpyAsync with a host
    operand reads the session's page-locked table image, in device-mode begin
    alone; the only other one is device to device, in the device-mode partner
    call; no stream-ordered allocation."""
    import build_native
    code = re.sub(r"//[^\n]*", "", open(os.path.join(build_native.CSRC, "parties_session.hip")).read())
    calls = list(re.finditer(r"\bhipMemcpy(?:2D)?Async\s*\(([^;]*)\);", code))
    assert len(calls) == 2
    for m in calls:
        owner = re.findall(r"^int (amph_parties_\w+)\(", code[:m.start()], re.M)[-1]
        if "hipMemcpyDeviceToDevice" in m.group(1):
            assert owner == "amph_parties_partner_dev"
        else:
            assert owner == "amph_parties_begin_dev" and "p->tables_host.p" in m.group(1)
    assert "hipMallocAsync" not in code
