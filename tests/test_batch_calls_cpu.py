"""Many secrets in one call (amph_*_packed / amph_*_batch), the parts that
need no GPU:

* the object lookup of the segmented kernels' failure path
  (amphora_amd/csrc/seglookup.hpp) compiled for the host and checked against a
  linear scan (tests/cpp/batch_test.cpp, mode `lookup`);
* the argument checks that return before any GPU work, on a context created
  without a GPU.
"""
import ctypes as C
import os
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


def test_lookup_matches_a_linear_scan():
    import build_native
    r = subprocess.run([build_native.build_batch_test(), "lookup"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "lookup ok" in r.stdout


@pytest.fixture(scope="module")
def L():
    import amphora_amd
    return amphora_amd._lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.Context(P, R, RINV)  # no HIP call until a launch


def _odos(L, n, words, nbytes=None):
    """n parties' ODO structs over zeroed host words (never read here)."""
    bufs = [np.zeros((5, max(1, words), 16), np.uint8) for _ in range(n)]
    arr = (L._AmphOdo * n)()
    for j in range(n):
        arr[j] = L._AmphOdo(*[bufs[j][k].ctypes.data for k in range(5)],
                            16 * words if nbytes is None else nbytes[j])
    return arr, bufs


def _packed(L, ctx, arr, n, offsets, K, flags=0, masked=False, words=4):
    off = np.asarray(offsets, dtype=np.uint64)
    out = np.zeros((max(1, words), 16), np.uint8)
    sec = np.zeros((max(1, words), 16), np.uint8)
    ff = np.full(max(1, K), 99, np.int64)
    if masked:
        st = L.lib.amph_mask_input_packed(ctx._h, arr, n, off.ctypes.data, K, sec.ctypes.data, out.ctypes.data,
                                          ff.ctypes.data, flags, None)
    else:
        st = L.lib.amph_recombine_verify_packed(ctx._h, arr, n, off.ctypes.data, K, out.ctypes.data,
                                                ff.ctypes.data, flags, None)
    return st, L.lib.amph_last_error().decode()


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("offsets", [[1, 2, 4], [0, 3, 2, 4], [0, 2, 3], [0, 2, 5]],
                         ids=["first-not-0", "decreasing", "last-below-words", "last-above-words"])
def test_packed_refuses_a_broken_host_table(L, ctx, masked, offsets):
    arr, keep = _odos(L, 2, 4)
    st, msg = _packed(L, ctx, arr, 2, offsets, len(offsets) - 1, masked=masked)
    assert st == E_PARAM and "offsets" in msg, (st, msg)


@pytest.mark.parametrize("masked", [False, True])
def test_packed_refuses_unequal_parties_and_host_io(L, ctx, masked):
    arr, keep = _odos(L, 2, 4, nbytes=[64, 48])
    st, msg = _packed(L, ctx, arr, 2, [0, 4], 1, masked=masked)
    assert st == E_LEN and "party 1" in msg, (st, msg)
    arr, keep = _odos(L, 2, 4)
    st, msg = _packed(L, ctx, arr, 2, [0, 4], 1, flags=F_HOST_IO, masked=masked)
    assert st == E_PARAM and "AMPH_F_HOST_IO" in msg, (st, msg)


def _batch(L, ctx, arr, n, K, flags=0, n_secrets=None, words=4):
    outs = [np.zeros((words, 16), np.uint8) for _ in range(max(1, K))]
    outp = (C.c_void_p * max(1, K))(*[x.ctypes.data for x in outs])
    ff = np.full(max(1, K), 99, np.int64)
    ffp = ff.ctypes.data_as(C.POINTER(C.c_int64))
    if n_secrets is None:
        st = L.lib.amph_recombine_verify_batch(ctx._h, arr, n, K, outp, ffp, flags)
    else:
        secs = [np.zeros((words, 16), np.uint8) for _ in range(max(1, K))]
        sp = (C.c_void_p * max(1, K))(*[x.ctypes.data for x in secs])
        ns = (C.c_size_t * max(1, K))(*n_secrets)
        st = L.lib.amph_mask_input_batch(ctx._h, arr, n, K, sp, ns, outp, ffp, flags)
    return st, L.lib.amph_last_error().decode()


@pytest.mark.parametrize("flags", [F_DEVICE, F_ACCUMULATE, F_HOST_IO])
def test_gather_refuses_every_flag(L, ctx, flags):
    arr, keep = _odos(L, 4, 4)  # 2 objects x 2 parties
    assert _batch(L, ctx, arr, 2, 2, flags=flags)[0] == E_PARAM
    assert _batch(L, ctx, arr, 2, 2, flags=flags, n_secrets=[4, 4])[0] == E_PARAM


def test_gather_names_the_object_with_the_wrong_secret_count(L, ctx):
    arr, keep = _odos(L, 6, 4)  # 3 objects x 2 parties, 4 words each
    st, msg = _batch(L, ctx, arr, 2, 3, n_secrets=[4, 3, 4])
    assert st == E_LEN and "object 1" in msg, (st, msg)
    st, msg = _batch(L, ctx, arr, 2, 3, n_secrets=[4, 4, 5])
    assert st == E_LEN and "object 2" in msg, (st, msg)


def test_gather_names_the_ragged_object(L, ctx):
    arr, keep = _odos(L, 4, 4, nbytes=[64, 64, 64, 60])
    st, msg = _batch(L, ctx, arr, 2, 2)
    assert st == E_LEN and "object 1" in msg, (st, msg)


def test_no_objects_is_ok(L, ctx):
    arr, keep = _odos(L, 2, 4)
    assert _packed(L, ctx, arr, 2, [0], 0)[0] == OK
    assert _packed(L, ctx, arr, 2, [0], 0, masked=True)[0] == OK
    assert _packed(L, ctx, arr, 2, [0], 0, flags=F_DEVICE)[0] == OK
    assert _batch(L, ctx, arr, 2, 0)[0] == OK
    assert _batch(L, ctx, arr, 2, 0, n_secrets=[0])[0] == OK


def test_python_mirror_exports_the_batch_calls(L):
    for name in ("recombine_verify_packed", "mask_input_packed", "recombine_verify_batch", "mask_input_batch"):
        assert callable(getattr(L.Context, name))
    from amphora_amd import client
    assert callable(client.verify_output_delivery_objects_batch) and callable(client.create_masked_inputs)
