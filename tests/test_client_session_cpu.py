"""The client session (include/amphora_client_session.h), the parts that need
no GPU: the extension header's own export list against the library's dynamic
symbols and the Python lists, and the entry points of the Python layers."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def L():
    import amphora_amd
    return amphora_amd._lib


def header_functions(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(amph_[a-z0-9_]+)\s*\(", src)))


def test_the_extension_header_has_its_own_export_list(L):
    names = header_functions("amphora_client_session.h")
    assert len(names) == 14 and all(n.startswith("amph_client_") for n in names)
    assert sorted(L.EXPORTED_CLIENT_SESSION) == names
    lib = C.CDLL(L.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), n
    # the library exports nothing of this family that the header does not declare
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r"\b(amph_client_[a-z0-9_]+)\b", nm))) == names
    others = (set(L.EXPORTED) | set(L.EXPORTED_WIRE_BATCH) | set(L.EXPORTED_UPLOAD_BATCH) |
              set(L.EXPORTED_RESPOND_BATCH) | set(L.EXPORTED_EXCHANGE_BATCH) | set(L.EXPORTED_PARTY_BATCH))
    assert not set(L.EXPORTED_CLIENT_SESSION) & others
    assert set(L.EXPORTED) == set(header_functions("amphora.h"))


def test_the_build_id_covers_the_new_unit():
    import build_native
    assert os.path.join(ROOT, "include", "amphora_client_session.h") in build_native.DEPS
    assert os.path.join(build_native.CSRC, "client_session.hip") in build_native.SOURCES


def test_the_python_entry_points_exist(L):
    from amphora_amd import client, loopback
    for name in ("client_begin", "client_begin_dev"):
        assert callable(getattr(L.Context, name))
    for name in ("party", "finish_verify", "finish_mask", "finish_mask_json", "word", "close"):
        assert callable(getattr(L.ClientSession, name))
    for name in ("add_body", "secret", "masked_input_json", "masked_input_body", "close"):
        assert callable(getattr(client.ResponseSession, name))
    with pytest.raises(ValueError):
        loopback.LoopbackAmphoraClient([], 0, 0, 0, transport="sessions")


def test_argument_checks_return_before_any_gpu_work(L):
    from oracle import amphora_oracle as O
    ctx = L.Context(O.TEST_PRIME, O.TEST_R, O.TEST_RINV)  # no HIP call until a launch
    h = C.c_void_p()
    assert L.lib.amph_client_begin(None, 1, 2, C.byref(h)) == L.AMPH_E_PARAM
    for n in (0, 17):
        assert L.lib.amph_client_begin(ctx._h, 1, n, C.byref(h)) == L.AMPH_E_PARAM and not h.value
        assert L.lib.amph_client_begin_dev(ctx._h, 1, n, None, C.byref(h)) == L.AMPH_E_PARAM
    assert L.lib.amph_client_begin(ctx._h, 1, 2, None) == L.AMPH_E_PARAM
    bad = C.c_int64()
    assert L.lib.amph_client_party(None, 0, None, C.byref(bad)) == L.AMPH_E_PARAM
    assert L.lib.amph_client_finish_verify(None, None, None, None) == L.AMPH_E_PARAM
    assert L.lib.amph_client_word(None, 0, None) == L.AMPH_E_PARAM
    assert L.lib.amph_client_words(None) == 0 and L.lib.amph_client_parties_seen(None) == 0
    L.lib.amph_client_free(None)
