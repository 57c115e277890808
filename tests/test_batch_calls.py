"""Many secrets in one call, one verdict per secret, on the GPU:
amph_recombine_verify_packed / amph_mask_input_packed (host and device mode)
and amph_recombine_verify_batch / amph_mask_input_batch (the gather form).

Expected values come from the C oracle, one object at a time -- never from
the library's own single calls.  The batch's object sizes put boundaries
inside a wave, on a wave edge and inside a 1,024-lane workgroup, with empty
objects at both ends and in the middle.
"""
import functools
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from oracle import amphora_oracle as O
from oracle import coracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, R, RINV = O.TEST_PRIME, O.TEST_R, O.TEST_RINV
NO_FAIL = 0x7F7F7F7F7F7F7F7F
SIZES = [0, 1, 0, 63, 64, 65, 1, 1, 1, 0, 130, 1025, 7, 0]  # 1,358 words
# object -> faulted local words: the 1-word object at position 1; the 65-word
# object twice (the smaller index wins); the first and third of the three
# adjacent 1-word objects, not the second; the last word of the 1,025-word
# object; word 0 of the 7-word object
FAULTS = {1: [0], 5: [3, 64], 6: [0], 8: [0], 11: [1024], 12: [0]}
FAULTS_2 = {5: [1], 10: [7], 11: [1024]}  # a second pass for AMPH_F_ACCUMULATE


@functools.lru_cache(maxsize=None)
def _field():
    return coracle.test_field(threads=4)


class Batch:
    """One batch: per-object ODOs with its own synth_odos call, the faults
    applied, and the oracle's results object by object."""

    def __init__(self, n, sizes, faults, seed):
        F = _field()
        self.n, self.sizes = n, list(sizes)
        self.objects, self.secrets, self.y, self.masked, self.ff = [], [], [], [], []
        for o, W in enumerate(sizes):
            if W == 0:
                e = np.zeros((0, 16), np.uint8)
                self.objects.append([tuple(e.copy() for _ in range(5)) for _ in range(n)])
                self.secrets.append(e.copy())
                self.y.append(e.copy())
                self.masked.append(e.copy())
                self.ff.append(-1)
                continue
            odos, _ = F.synth_odos(seed=seed + 31 * o, n=n, W=W, noncanon_permille=200)
            odos = [tuple(np.ascontiguousarray(f).copy() for f in p) for p in odos]
            for i in faults.get(o, []):
                odos[n - 1][3][i, 0] ^= 1  # <w> of the last party: w != y r at word i
            sec = F.synth_words(seed=seed + 31 * o + 7, count=W, mont=False)
            y, ff = F.recombine_verify(odos)
            m, mff = F.mask_input(sec, odos)
            assert ff == mff == (min(faults[o]) if o in faults else -1), "the fixture's faults"
            self.objects.append(odos)
            self.secrets.append(sec)
            self.y.append(y)
            self.masked.append(m)
            self.ff.append(int(ff))
        self.offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
        self.packed = [tuple(np.ascontiguousarray(np.concatenate([self.objects[o][j][k] for o in range(len(sizes))]))
                             for k in range(5)) for j in range(n)]
        self.packed_secrets = np.ascontiguousarray(np.concatenate(self.secrets))
        self.packed_y = np.concatenate(self.y)
        self.packed_masked = np.concatenate(self.masked)
        for a in (self.packed_y, self.packed_masked, self.packed_secrets, self.offsets):
            a.setflags(write=False)

    def check_packed(self, out, ff, masked):
        assert list(np.asarray(ff, dtype=np.int64)) == self.ff
        assert np.array_equal(np.asarray(out), self.packed_masked if masked else self.packed_y)

    def check_pieces(self, outs, ff, masked):
        assert list(np.asarray(ff, dtype=np.int64)) == self.ff
        exp = self.masked if masked else self.y
        assert len(outs) == len(exp)
        for got, want in zip(outs, exp):
            assert got.shape == want.shape and np.array_equal(got, want)


@functools.lru_cache(maxsize=None)
def batch(n, faulted):
    return Batch(n, SIZES, FAULTS if faulted else {}, seed=1000 + n)


@pytest.fixture(scope="module")
def A():
    import amphora_amd
    return amphora_amd


@pytest.fixture(scope="module")
def ctx(A):
    return A.Context(P, R, RINV)


def _dev(x):
    import torch
    x = np.array(x, copy=True)  # the fixtures are read-only
    return torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).cuda()


def _dev_verdicts(ff):
    """A device verdict array as the host form's: AMPH_NO_FAILURE -> -1."""
    import torch
    torch.cuda.synchronize()
    v = ff.cpu().numpy()
    return np.where(v == NO_FAIL, -1, v)


def run_form(ctx, b, form, masked):
    if form == "packed_host":
        if masked:
            out, ff = ctx.mask_input_packed(b.packed, b.offsets, b.packed_secrets)
        else:
            out, ff = ctx.recombine_verify_packed(b.packed, b.offsets)
        b.check_packed(out, ff, masked)
    elif form == "packed_device":
        d = [tuple(_dev(f) for f in p) for p in b.packed]
        off = _dev(b.offsets)
        if masked:
            out, ff = ctx.mask_input_packed(d, off, _dev(b.packed_secrets))
        else:
            out, ff = ctx.recombine_verify_packed(d, off)
        v = _dev_verdicts(ff)
        b.check_packed(out.cpu().numpy(), v, masked)
    else:
        if masked:
            outs, ff = ctx.mask_input_batch(b.objects, b.secrets)
        else:
            outs, ff = ctx.recombine_verify_batch(b.objects)
        b.check_pieces(outs, ff, masked)


FORMS = ["packed_host", "packed_device", "gather"]


@pytest.mark.parametrize("masked", [False, True], ids=["verify", "mask"])
@pytest.mark.parametrize("faulted", [False, True], ids=["honest", "faulted"])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_batch_matches_the_oracle_per_object(ctx, n, form, faulted, masked):
    run_form(ctx, batch(n, faulted), form, masked)


def test_status_and_message_of_a_faulted_batch(A, ctx):
    b = batch(2, True)
    arr, keep = ctx._odo_structs(b.packed)
    out, ff = np.empty((int(b.offsets[-1]), 16), np.uint8), np.empty(len(SIZES), np.int64)
    st = A._lib.lib.amph_recombine_verify_packed(ctx._h, arr, 2, b.offsets.ctypes.data, len(SIZES),
                                                 out.ctypes.data, ff.ctypes.data, 0, None)
    msg = A._lib.lib.amph_last_error().decode()
    assert st == A._lib.AMPH_E_VERIFY and "object 1 " in msg and "6 of 14 objects" in msg, (st, msg)


@pytest.mark.parametrize("form", FORMS)
def test_grid_stride_and_small_blocks(A, monkeypatch, form):
    """64-lane workgroups under a grid cap of 3: 192 lanes stride over 1,358 words."""
    monkeypatch.setenv("AMPH_BLOCK", "64")
    monkeypatch.setenv("AMPH_GRID_CAP", "3")
    c = A.Context(P, R, RINV)
    for faulted in (False, True):
        for masked in (False, True):
            run_form(c, batch(2, faulted), form, masked)


@functools.lru_cache(maxsize=None)
def pipeline_batch():
    # faults in objects 0, 17 and 39; with 4,096-word batches object 17
    # ([17000, 18000)) lies inside one pipeline batch, so object 20
    # ([20000, 21000), batch boundary at 20480) also carries one, at a word of
    # a later pipeline batch than its first word
    return Batch(2, [1000] * 40, {0: [5], 17: [900], 20: [900], 39: [999]}, seed=77)


@pytest.mark.parametrize("form", ["packed_host", "gather"])
def test_host_pipeline_across_batches(A, monkeypatch, form):
    monkeypatch.setenv("AMPH_SMALL_BYTES", "0")
    c = A.Context(P, R, RINV)
    c.set_batch_words(4096)
    b = pipeline_batch()
    before = c.stats()["kernel_launches"]
    run_form(c, b, form, False)
    assert c.stats()["kernel_launches"] - before == 10  # ceil(40,000 / 4,096) batches
    run_form(c, b, form, True)


def test_accumulate_min_combines_per_object(A, ctx):
    import torch
    b1, b2 = batch(2, True), Batch(2, SIZES, FAULTS_2, seed=1002)
    off = _dev(b1.offsets)
    for masked in (False, True):
        ff = torch.full((len(SIZES),), NO_FAIL, dtype=torch.int64, device="cuda")
        for b in (b1, b2):
            d = [tuple(_dev(f) for f in p) for p in b.packed]
            if masked:
                ctx.mask_input_packed(d, off, _dev(b.packed_secrets), first_fail=ff, accumulate=True)
            else:
                ctx.recombine_verify_packed(d, off, first_fail=ff, accumulate=True)
        want = [min([x for x in (u, v) if x >= 0], default=-1) for u, v in zip(b1.ff, b2.ff)]
        assert want[5] == 1 and want[10] == 7 and want[1] == 0  # both passes show
        assert list(_dev_verdicts(ff)) == want


@pytest.mark.parametrize("form", FORMS)
def test_multi_device_context(A, form):
    c = A.Context(P, R, RINV, devices=[0, 0])
    assert c.device_count == 2
    for masked in (False, True):
        run_form(c, batch(2, True), form, masked)


def test_empty_words_read_verified(ctx):
    """T = 0 with objects: every verdict reads "verified", nothing is launched."""
    e = np.zeros((0, 16), np.uint8)
    before = ctx.stats()["kernel_launches"]
    out, ff = ctx.recombine_verify_packed([(e, e, e, e, e)] * 2, np.zeros(4, np.uint64))
    assert out.shape == (0, 16) and list(ff) == [-1, -1, -1]
    outs, ff = ctx.mask_input_batch([[(e, e, e, e, e)] * 2] * 3, [e] * 3)
    assert list(ff) == [-1, -1, -1] and ctx.stats()["kernel_launches"] == before


# ------------------------------------------------------------------ Python mirror
def _odo_objects(A, b):
    return [[A.OutputDeliveryObject(*[f.tobytes() for f in party]) for party in obj] for obj in b.objects]


def _reference_message(b, o):
    util = O.ClientSecretShareUtil(P, R, RINV)
    vals = [util.recombine_object([party[k].tobytes() for party in b.objects[o]]) for k in range(5)]
    y, r, v, w, u = vals
    return O.verification_failure_message(P, b.ff[o], y, r, u, v, w)


def test_python_mirror_one_entry_per_secret(A, ctx):
    from amphora_amd import client
    util = client.SecretShareUtil(ctx)
    b = batch(2, True)
    res = client.verify_output_delivery_objects_batch(util, _odo_objects(A, b))
    assert len(res) == len(SIZES)
    for o, r in enumerate(res):
        if b.ff[o] < 0:
            assert r == client.unpack(b.y[o])
        else:
            assert isinstance(r, A.IntegrityVerificationException)
            assert str(r) == _reference_message(b, o)
    secrets = [A.Secret.of([], client.unpack(s)) for s in b.secrets]
    res = client.create_masked_inputs(util, secrets, _odo_objects(A, b))
    for o, r in enumerate(res):
        if b.ff[o] < 0:
            assert r.secret_id == secrets[o].secret_id
            assert np.array_equal(np.asarray(r.data.words).reshape(-1, 16), b.masked[o])
        else:
            assert isinstance(r, A.IntegrityVerificationException) and str(r) == _reference_message(b, o)


def test_python_mirror_routes_odd_objects_through_the_single_call(A, ctx):
    from amphora_amd import client
    util = client.SecretShareUtil(ctx)
    b = batch(2, False)
    objs = _odo_objects(A, b)
    secrets = [A.Secret.of([], client.unpack(s)) for s in b.secrets]
    secrets[4] = A.Secret.of([], client.unpack(b.secrets[4]) + [5])  # 65 secrets for 64 masks
    secrets[10] = A.Secret.of([], client.unpack(b.secrets[10])[:100])  # fewer secrets than masks
    with pytest.raises(IndexError) as single:
        client.create_masked_input(util, secrets[4], objs[4])
    res = client.create_masked_inputs(util, secrets, objs)
    assert type(res[4]) is type(single.value) and str(res[4]) == str(single.value) == \
        "Index 64 out of bounds for length 64"
    assert np.array_equal(np.asarray(res[10].data.words), b.masked[10][:100])
    for o in (3, 5, 11):
        assert np.array_equal(np.asarray(res[o].data.words).reshape(-1, 16), b.masked[o])
    # a ragged object (party 1 one word short: that word reads as zeros) keeps the single call's verdict
    short = A.OutputDeliveryObject(*[f.tobytes()[:-16] for f in b.objects[5][1]])
    ragged = [objs[5][0], short]
    with pytest.raises(A.IntegrityVerificationException) as single:
        client.verify_output_delivery_objects(util, ragged)
    res = client.verify_output_delivery_objects_batch(util, [objs[3], ragged, objs[12]])
    assert res[0] == client.unpack(b.y[3]) and res[2] == client.unpack(b.y[12])
    assert isinstance(res[1], A.IntegrityVerificationException) and str(res[1]) == str(single.value)


# --------------------------------------------------------------------- C++ mirror
@pytest.mark.parametrize("faulted", [False, True], ids=["honest", "faulted"])
def test_cpp_mirror_batch(tmp_path, faulted):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import build_native
    b = batch(2, faulted)
    path = tmp_path / "batch.bin"
    with open(path, "wb") as fh:
        fh.write(struct.pack("<QQ", b.n, len(SIZES)))
        for x in (P, R, RINV):
            fh.write(int(x).to_bytes(16, "little"))
        for o, W in enumerate(SIZES):
            fh.write(struct.pack("<Qq", W, b.ff[o]))
            for party in b.objects[o]:
                for f in party:
                    fh.write(np.ascontiguousarray(f).tobytes())
            for a in (b.y[o], b.secrets[o], b.masked[o]):
                fh.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([build_native.build_batch_test(), "gpu", str(path)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "gpu ok" in r.stdout, r.stdout + r.stderr
