"""The client session for K secrets (include/amphora_client_batch.h), the
parts that need no GPU: the extension header's own export list against the
library's dynamic symbols and the Python lists, the entry points of the Python
layers, the argument checks that return before any GPU work, the host-copy
ordering rule in the new unit, and a plain-Python model of per-object running
sums and per-object verdicts that agrees with the ``%`` references and, with
ONE planted error (a tile that adds into the next object's words), disagrees.
"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import field_cases as FC

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
    names = header_functions("amphora_client_batch.h")
    assert len(names) == 20 and all(n.startswith("amph_clients_") for n in names)
    assert sorted(L.EXPORTED_CLIENTS_SESSION) == names
    lib = C.CDLL(L.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), n
    # the library exports nothing of this family that the header does not declare
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r"\b(amph_clients_[a-z0-9_]+)\b", nm))) == names
    others = (set(L.EXPORTED) | set(L.EXPORTED_WIRE_BATCH) | set(L.EXPORTED_UPLOAD_BATCH) |
              set(L.EXPORTED_RESPOND_BATCH) | set(L.EXPORTED_EXCHANGE_BATCH) | set(L.EXPORTED_PARTY_BATCH) |
              set(L.EXPORTED_CLIENT_SESSION))
    assert not set(L.EXPORTED_CLIENTS_SESSION) & others
    assert set(L.EXPORTED) == set(header_functions("amphora.h"))
    # K-entry verdict arrays: no prototype here spells a parameter `first_fail` (the
    # verdict matrix of tests/verdict_cases.py is keyed by that spelling)
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "amphora_client_batch.h")).read(), flags=re.S)
    assert not re.search(r"\bfirst_fail\b", src) and not re.search(r"\bbad_char\b", src)
    assert len(re.findall(r"int64_t\s*\*\s*first_fails\b", src)) == 6


def test_the_build_id_covers_the_new_unit():
    import build_native
    assert os.path.join(ROOT, "include", "amphora_client_batch.h") in build_native.DEPS
    assert os.path.join(build_native.CSRC, "clients_session.hip") in build_native.SOURCES
    # not a capi_* unit: tests/test_host_ordering.py pins that set
    assert not [f for f in os.listdir(build_native.CSRC) if f.startswith("capi") and "clients" in f]


def test_the_python_entry_points_exist(L):
    from amphora_amd import client, loopback
    for name in ("clients_begin", "clients_begin_dev", "clients_copies"):
        assert callable(getattr(L.Context, name))
    for name in ("party", "party_texts", "finish_verify", "finish_mask", "finish_mask_json", "word", "close",
                 "pack_texts", "split_upload"):
        assert callable(getattr(L.ClientSessions, name))
    for name in ("add_bodies", "secrets", "masked_input_bodies", "close"):
        assert callable(getattr(client.ResponseSessions, name))
    for name in ("get_secrets", "create_secrets"):
        assert callable(getattr(loopback.LoopbackAmphoraClient, name))
    with pytest.raises(ValueError):  # no new transport name
        loopback.LoopbackAmphoraClient([], 0, 0, 0, transport="sessions")


def test_argument_checks_return_before_any_gpu_work(L):
    from oracle import amphora_oracle as O
    ctx = L.Context(O.TEST_PRIME, O.TEST_R, O.TEST_RINV)  # no HIP call until a launch
    lib, E_PARAM = L.lib, L.AMPH_E_PARAM
    tab = lambda *w: np.asarray(w, np.uint64)  # noqa: E731
    ok = tab(0, 3, 5)
    for dev in (False, True):
        def begin(c, wo, K, n, out=True):
            h = C.c_void_p()
            args = [c, None if wo is None else wo.ctypes.data, K, n]
            st = (lib.amph_clients_begin_dev(*args, None, C.byref(h) if out else None) if dev else
                  lib.amph_clients_begin(*args, C.byref(h) if out else None))
            assert not h.value
            return st, lib.amph_last_error().decode()
        for args, word in [((None, ok, 2, 2), "null context"), ((ctx._h, None, 2, 2), "null word_offsets"),
                           ((ctx._h, ok, 2, 0), "n_parties must be in [1, 16]"),
                           ((ctx._h, ok, 2, 17), "n_parties must be in [1, 16]"),
                           ((ctx._h, ok, 0, 2), "at least one object"),
                           ((ctx._h, tab(1, 3, 5), 2, 2), "word_offsets[0] must be 0"),
                           ((ctx._h, tab(0, 6, 5), 2, 2), "nondecreasing (object 1)")]:
            st, msg = begin(*args)
            assert st == E_PARAM and word in msg, (dev, word, st, msg)
        assert begin(ctx._h, ok, 2, 2, out=False)[0] == E_PARAM
    v = np.zeros(8, np.int64)
    p = v.ctypes.data
    for st in (lib.amph_clients_party(None, 0, None, p), lib.amph_clients_party_dev(None, 0, None, p, None),
               lib.amph_clients_finish_verify(None, None, p, p), lib.amph_clients_finish_verify_dev(None, None, p, p, None),
               lib.amph_clients_finish_mask(None, None, None, None, p, p),
               lib.amph_clients_finish_mask_dev(None, None, None, None, p, p, None),
               lib.amph_clients_finish_mask_json(None, None, None, 0, p, p),
               lib.amph_clients_finish_mask_json_dev(None, None, None, 0, p, p, None),
               lib.amph_clients_word(None, 0, 0, None), lib.amph_clients_field_offsets(None, p),
               lib.amph_clients_upload_offsets(None, p)):
        assert st == E_PARAM and "null client batch session" in lib.amph_last_error().decode()
    assert lib.amph_clients_objects(None) == 0 and lib.amph_clients_words(None) == 0
    assert lib.amph_clients_field_chars(None) == 0 and lib.amph_clients_upload_chars(None) == 0
    assert lib.amph_clients_parties_seen(None) == 0 and lib.amph_clients_copies(None) == 0
    assert lib.amph_clients_copies(ctx._h) == 0
    lib.amph_clients_free(None)
    assert ctx.stats()["kernel_launches"] == 0
    with pytest.raises(L.AmphoraNativeError, match="nondecreasing"):
        ctx.clients_begin([0, 6, 5], 2)


def test_the_sessions_async_copies_keep_the_host_ordering_rule():
    """The host-copy ordering rule (tests/test_host_ordering.py states it for
    the capi_* units) in this family's unit: the one hipMemcpyAsync with a host
    operand reads the session's page-locked table image, in begin's device
    branch; the only other one is device to device, the K bad-character words
    of a device-mode finish; no stream-ordered allocation.  The shared host
    image (BatchImage, capi_internal.hpp) copies with blocking hipMemcpy only."""
    import build_native
    code = re.sub(r"//[^\n]*", "", open(os.path.join(build_native.CSRC, "clients_session.hip")).read())
    calls = list(re.finditer(r"\bhipMemcpy(?:2D)?Async\s*\(([^;]*)\);", code))
    assert len(calls) == 2
    for m in calls:
        owner = re.findall(r"^int (clients_\w+)\(", code[:m.start()], re.M)[-1]
        if "hipMemcpyDeviceToDevice" in m.group(1):
            assert owner == "clients_finish_dev" and "p->d_bad" in m.group(1)
        else:
            assert owner == "clients_begin" and "p->tables_host.p" in m.group(1)
            assert "if (dev) {" in code[:m.start()].rsplit("hipError_t e = hipSuccess;", 1)[1]
    assert "hipMallocAsync" not in code
    internal = re.sub(r"//[^\n]*", "", open(os.path.join(build_native.CSRC, "capi_internal.hpp")).read())
    image = internal[internal.index("struct BatchImage"):]
    assert "Async(" not in image.replace("hipMemsetAsync(", "") and "hipMemcpy(dst + from" in image
    # wire_batch_status is shared, not restated
    batch = open(os.path.join(build_native.CSRC, "capi_batch.hip")).read()
    unit = open(os.path.join(build_native.CSRC, "clients_session.hip")).read()
    assert "inline int wire_batch_status(" in internal
    for src in (batch, unit):
        assert "wire_batch_status(" in src and "int wire_batch_status(" not in src


# ---- a Python model of per-object running sums and verdicts ---------------------------------
TILE = 4  # the model's tile (the kernel's is 192 words): several tiles per object on the rows' 100-odd words


def model_tiles(woff):
    """(object, local tile) of every workgroup, by the ownership rule of
    csrc/wiretiles.hpp: g(o) = woff[o] // t + o, the LAST o with g(o) <= w."""
    K, T = len(woff) - 1, woff[-1]
    out = []
    for w in range(T // TILE + K):
        o = max(o for o in range(K) if woff[o] // TILE + o <= w)
        local = w - (woff[o] // TILE + o)
        if local < -(-(woff[o + 1] - woff[o]) // TILE):
            out.append((o, local))
    return out


def model_clients(pr, rows, woff, order, bug=None):
    """-> (sums[k][T], first_fails[K]).  Every party's launch walks the tiles;
    a tile of object o adds its canonical words into sums[k][woff[o] + word].
    Planted `next_object`: an object's LAST tile uses the next object's base."""
    K, T = len(woff) - 1, woff[-1]
    sums = [[0] * T for _ in range(5)]
    for j in order:
        for o, local in model_tiles(woff):
            W = woff[o + 1] - woff[o]
            last = local == -(-W // TILE) - 1
            base = woff[o + 1] if bug == "next_object" and last and o + 1 < K else woff[o]
            for i in range(local * TILE, min(W, (local + 1) * TILE)):
                for k in range(5):
                    at = base + i
                    if at < T:
                        sums[k][at] = (sums[k][at] + rows.odos[j][k][woff[o] + i] % pr.p) % pr.p
    Rinv = pow(FC.M128, -1, pr.p)
    ffs = []
    for o in range(K):
        ff = -1
        for i in range(woff[o], woff[o + 1]):
            if sums[0][i] * sums[1][i] * Rinv % pr.p != sums[3][i] or sums[2][i] * sums[1][i] * Rinv % pr.p != sums[4][i]:
                ff = i - woff[o]  # counted from the object's own first word
                break
        ffs.append(ff)
    return sums, ffs


def tables_for(W):
    return [[0, W], [0, 0, 1, TILE + 1, TILE + 1, 3 * TILE + 1, W, W], [0, W // 3, 2 * W // 3, W]]


def test_every_tile_has_one_owner_in_the_model():
    for woff in tables_for(101):
        seen = model_tiles(woff)
        want = [(o, t) for o in range(len(woff) - 1) for t in range(-(-(woff[o + 1] - woff[o]) // TILE))]
        assert sorted(seen) == want and len(set(seen)) == len(seen)


@pytest.mark.parametrize("pid", FC.PRIME_IDS)
def test_the_model_agrees_with_the_references_and_the_planted_error_does_not(pid):
    pr = FC.BY_ID[pid]
    for n in (2, 3):
        rows = FC.odo_rows(pid, n)
        for woff in tables_for(rows.W):
            for order in FC.session_orders(n):
                want = FC.running_sums(pr, rows, order)
                sums, ffs = model_clients(pr, rows, woff, order)
                assert sums == want and ffs == [-1] * (len(woff) - 1), (n, woff, order)
                assert [FC.from_gfp(pr, x) for x in sums[0]] == list(rows.ys)
                bad_sums, bad_ffs = model_clients(pr, rows, woff, order, bug="next_object")
                if len(woff) > 2:
                    assert bad_sums != want and any(f >= 0 for f in bad_ffs), (n, woff, order)
                else:  # one object has no neighbour to spill into
                    assert bad_sums == want
    # a fault in one object: its own verdict alone, with its own index
    rows = FC.odo_rows(pid, 2)
    woff = tables_for(rows.W)[2]
    hit = woff[1] + 2
    odos = [[list(f) for f in o] for o in rows.odos]
    odos[0][3][hit] += 1 if odos[0][3][hit] < FC.MASK128 else -1  # off by one without wrapping, as FC.with_fault
    faulty = FC.Rows(rows.W, 2, tuple(tuple(tuple(f) for f in o) for o in odos), *rows[3:])
    assert model_clients(pr, faulty, woff, [1, 0])[1] == [-1, 2, -1]
