"""Many secrets in one call: what the segmented kernels cost on the hot path
and what batching buys ("Packed calls").

    python tools/bench_batch.py [--reps R] [--out FILE]
    python tools/bench_batch.py --wire [--variant-lib LIB] [--reps R] [--out FILE]
    python tools/bench_batch.py --upload [--reps R] [--out FILE]
    python tools/bench_batch.py --respond [--reps R] [--out FILE]
    python tools/bench_batch.py --exchange [--reps R] [--out FILE]
    python tools/bench_batch.py --exchange-single --parent-lib LIB [--parent-lib-copy LIB2] [--reps R] [--out FILE]

GPU only (fails without a device).  Everything is warmed up, then timed in
alternating order within this one process; one JSON line with the build id.

* hot path: k_rv / k_mask against k_rv_seg / k_mask_seg at 2^20 words x 2
  parties, honest input, with a one-object table and with 1,024 objects of
  1,024 words; kernel time from events stamped by the dispatch itself
  (amph_time_next_launch).  k_rv / k_mask are also timed against themselves
  (series a and a2 of each round): the run's spread.
* batching: 256 objects x 1,000 words x 2 parties.  Host mode: one
  amph_*_batch call against 256 single calls.  Device mode: one packed call
  against 256 enqueued device calls, each side ending in one synchronise.
  Wall clock around the C ABI calls (prebuilt arguments).
* worst case: the segmented kernels at 2^20 words with EVERY word failing
  (recorded, not bounded), beside k_rv / k_mask on the same input.

--wire measures the many-secrets wire-text calls instead (DESIGN.md section
4c', include/amphora_wire_batch.h), same method:

* hot path: k_rv_b64 / k_mask_b64 on one text of 2^20 words x 2 parties (timed
  twice per round: the spread) against k_rv_b64_seg / k_mask_b64_seg with 1
  object, 1,024 objects of 1,024 words and 1,049 objects of 1,000 words.
* last tile (with --variant-lib: a second library built from the same tree
  with -DAMPH_WIRE_SEG_LANES=0, the whole-tile per-character path): the two
  forms at 1,000-word and 100-word objects, the default form twice per round.
* batching: 256 objects x 1,000 words x 2 parties, host mode, wall clock with
  prebuilt arguments: the batch call, 256 single wire-text calls, and 5 n
  field decodes per object followed by the packed word call; and the same
  size in device mode (one packed call against 256 enqueued single calls).

--upload measures the many-uploads calls (DESIGN.md section 4c'',
include/amphora_upload_batch.h), same method, one run on one board:

* batching: 256 uploads x 1,000 words.  Client side at 2 and 3 parties: the
  host batch call (amph_mask_input_json_batch) against 256 single host calls
  (amph_mask_input_json), the device packed call against 256 enqueued single
  device calls.  Party side: amph_convert_share_json_batch / _packed against
  256 amph_convert_share_json calls, on the texts the client side wrote.
* hot path at ONE object of the same 256,000 words, kernel time: k_mask_json
  (twice per round: the spread) against k_mask_json_seg at 2 and 3 parties,
  k_conv_json (twice) against k_conv_json_seg.

--respond measures the many-responses call (DESIGN.md section 4c''',
include/amphora_respond_batch.h), same method, one run on one board:

* batching: 256 objects x 1,000 words.  Device: one amph_odo_fields_b64_packed
  call against 5 x 256 enqueued amph_base64_encode device calls, one
  synchronise per side.  Host: amph_odo_fields_b64_batch and _packed against
  5 x 256 host amph_base64_encode calls.
* hot path at ONE object of the same 256,000 words, kernel time: k_odo_b64_seg
  against the SUM of the five k_b64_encode_blk launches amph_base64_encode makes
  for the five fields, that sum taken twice per round (a, a2: the spread).

--exchange measures the many-requests exchange codec calls (DESIGN.md section
4c'''', include/amphora_exchange_batch.h), same method, one run on one board:

* batching: 256 objects x 2,000 pairs of full-length diffs, 3 parties' worth of
  texts per round (one encode, two partners' decodes).  One
  amph_exchange_encode_packed and two amph_exchange_decode_packed calls
  against 256 amph_exchange_encode and 512 amph_exchange_decode calls, device
  mode (one synchronise per side) and host mode.
* hot path at ONE object of 512,000 pairs, kernel time from the call's first
  launch to its last: each packed call against its single call, the single
  call twice per round (a, a2: the spread).

--exchange-single measures what the many-requests change costs the SINGLE
exchange calls: amph_exchange_encode / amph_exchange_decode at 8 Mi pairs from
this tree's library and from another build's (--parent-lib: the parent
commit's libamphora_hip.so, built from a checkout of it) loaded side by side,
rows rotating through the round, the other build twice per round, and with
--parent-lib-copy the same bytes loaded once more from another path.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_batch.py measures on the GPU only: no device found")

import amphora_amd as A  # noqa: E402
from amphora_amd.spdz import TEST_PRIME, TEST_R, TEST_RINV  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default=None, help="also write the JSON line to this file")
ap.add_argument("--wire", action="store_true", help="the many-secrets wire-text calls (section 4c')")
ap.add_argument("--upload", action="store_true", help="the many-uploads calls (section 4c'')")
ap.add_argument("--respond", action="store_true", help="the many-responses call (section 4c''')")
ap.add_argument("--exchange", action="store_true", help="the many-requests exchange codec calls (section 4c'''')")
ap.add_argument("--exchange-single", action="store_true",
                help="the single exchange calls at 8 Mi pairs, this tree against --parent-lib")
ap.add_argument("--parent-lib", default=None, help="--exchange-single: another build's libamphora_hip.so")
ap.add_argument("--parent-lib-copy", default=None, help="--exchange-single: a copy of --parent-lib under another path")
ap.add_argument("--variant-lib", default=None, help="--wire: a library built with -DAMPH_WIRE_SEG_LANES=0")
a = ap.parse_args()

_lib = A._lib
L = _lib.lib
ctx = A.Context(TEST_PRIME, TEST_R, TEST_RINV)
N = 2
i64p = C.POINTER(C.c_int64)


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": round(statistics.median(ts), 5), "min_ms": round(ts[0], 5),
            "p25_ms": round(ts[len(ts) // 4], 5), "p75_ms": round(ts[(3 * len(ts)) // 4], 5),
            "max_ms": round(ts[-1], 5)}


def alternate(rows, reps, warmup, measure):
    """rows: name -> callable; every round runs each row once, in order."""
    ts = {k: [] for k in rows}
    for r in range(reps + warmup):
        for k, fn in rows.items():
            t = measure(fn)
            if r >= warmup:
                ts[k].append(t)
    return {k: stats(v) for k, v in ts.items()}


ev = [_lib.TimingEvent(), _lib.TimingEvent()]


def kernel_ms(fn):
    L.amph_time_next_launch(ev[0].handle, ev[1].handle)
    fn()
    torch.cuda.synchronize()
    return ev[0].elapsed_ms(ev[1])


def wall_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def ratio(res, num, den):
    return round(res[num]["median_ms"] / res[den]["median_ms"], 4)


def emit(result):
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


def slotted(field, K, WO):
    """field (T, 16) device words -> one buffer with K objects' own base64
    texts of WO words each ('=' padded), dense slots, '!' in the gaps."""
    nb, nc, sl = 16 * WO, _lib.wire_text_chars(WO), _lib.wire_slot_chars(WO)
    pad = -nb % 3
    x = torch.nn.functional.pad(field[:K * WO].reshape(K, nb), (0, pad)).reshape(-1).contiguous()
    enc = ctx.base64_encode(x).reshape(K, nc)
    if pad:
        enc[:, nc - pad:] = ord("=")
    buf = torch.full((K, sl), ord("!"), dtype=torch.uint8, device="cuda")
    buf[:, :nc] = enc
    return buf.reshape(-1)


def b64_structs(bufs, nchars, off=0, ptr=lambda x: x.data_ptr(), n=N):
    return (_lib._AmphOdoB64 * n)(*[_lib._AmphOdoB64(*[ptr(bufs[k][j]) + off for k in range(5)], nchars)
                                    for j in range(n)])


# ---------------------------------------------------------------- --wire
def wire_mode():
    F_DEV = _lib.AMPH_F_DEVICE
    stream = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    nchars_of, slot_of = _lib.wire_text_chars, _lib.wire_slot_chars

    def ok(st, lib=L):
        if st != 0:
            raise RuntimeError(lib.amph_last_error().decode())

    def table(K, WO):
        woff = torch.arange(0, K * WO + 1, WO, dtype=torch.int64, device="cuda")
        toff = torch.arange(0, K * slot_of(WO), slot_of(WO), dtype=torch.int64, device="cuda")
        return woff, toff

    class Shape:  # K objects of WO words as slotted device texts + the call's arguments
        def __init__(self, field_bufs, secrets, K, WO):
            self.K, self.WO, self.T = K, WO, K * WO
            self.bufs = [[slotted(field_bufs[k, j], K, WO) for j in range(N)] for k in range(5)]
            self.arr = b64_structs(self.bufs, K * slot_of(WO))
            self.woff, self.toff = table(K, WO)
            self.sec = secrets
            self.ff = torch.empty(K, dtype=torch.int64, device="cuda")
            self.bad = torch.empty(K, dtype=torch.int64, device="cuda")
            self.o16 = torch.empty((self.T, 16), dtype=torch.uint8, device="cuda")
            self.o24 = torch.empty((self.T, 24), dtype=torch.uint8, device="cuda")

        def rv(self, lib=L, h=None):
            ok(lib.amph_recombine_verify_b64_packed(h or ctx._h, self.arr, N, self.woff.data_ptr(),
                                                    self.toff.data_ptr(), self.K, self.o16.data_ptr(),
                                                    self.ff.data_ptr(), self.bad.data_ptr(), F_DEV, stream), lib)

        def mask(self, lib=L, h=None):
            ok(lib.amph_mask_input_b64_packed(h or ctx._h, self.arr, N, self.woff.data_ptr(), self.toff.data_ptr(),
                                              self.K, self.sec.data_ptr(), self.o16.data_ptr(), self.o24.data_ptr(),
                                              self.ff.data_ptr(), self.bad.data_ptr(), F_DEV, stream), lib)

        def clean(self):
            torch.cuda.synchronize()
            return bool((self.ff == _lib.AMPH_NO_FAILURE).all()) and bool((self.bad == _lib.AMPH_NO_FAILURE).all())

    W = 1 << 20
    WMAX = 1049 * 1000
    _, buf, _ = ctx.synth_odos(11, N, WMAX, noncanon_permille=20)  # (5, N, WMAX, 16)
    secrets = ctx.synth_words(12, WMAX)
    result = {"tool": "bench_batch --wire", "build_id": _lib.check_build_id(),
              "device": torch.cuda.get_device_name(0), "parties": N, "reps": a.reps, "warmup": a.warmup}

    # hot path: the unsegmented kernels on one text against the segmented ones
    one = Shape(buf, secrets, 1, W)  # one object: the single call's own text and layout
    s1024, s1000 = Shape(buf, secrets, 1024, 1024), Shape(buf, secrets, 1049, 1000)
    flat = b64_structs(one.bufs, nchars_of(W))
    ff1 = torch.empty(1, dtype=torch.int64, device="cuda")
    bad1 = torch.empty(1, dtype=torch.int64, device="cuda")

    def rv_flat():
        ok(L.amph_recombine_verify_b64(ctx._h, flat, N, W, one.o16.data_ptr(),
                                       C.cast(C.c_void_p(ff1.data_ptr()), i64p),
                                       C.cast(C.c_void_p(bad1.data_ptr()), i64p), F_DEV, stream))

    def mask_flat():
        ok(L.amph_mask_input_b64(ctx._h, flat, N, W, secrets.data_ptr(), W, one.o16.data_ptr(), one.o24.data_ptr(),
                                 C.cast(C.c_void_p(ff1.data_ptr()), i64p),
                                 C.cast(C.c_void_p(bad1.data_ptr()), i64p), F_DEV, stream))

    hot = {}
    for name, flat_fn, seg in (("k_rv_b64", rv_flat, "rv"), ("k_mask_b64", mask_flat, "mask")):
        res = alternate({name + "_a": flat_fn,
                         name + "_seg_1_object": getattr(one, seg),
                         name + "_seg_1024x1024": getattr(s1024, seg),
                         name + "_seg_1049x1000": getattr(s1000, seg),
                         name + "_a2": flat_fn}, a.reps, a.warmup, kernel_ms)
        assert one.clean() and s1024.clean() and s1000.clean() and int(ff1.item()) == _lib.AMPH_NO_FAILURE
        per_word = lambda k, words: res[k]["median_ms"] / words  # noqa: E731
        res["ratios"] = {
            name + "_a2_over_a (spread)": ratio(res, name + "_a2", name + "_a"),
            name + "_seg_1_object_over_flat": ratio(res, name + "_seg_1_object", name + "_a"),
            name + "_seg_1024x1024_over_flat": ratio(res, name + "_seg_1024x1024", name + "_a"),
            name + "_seg_1049x1000_over_flat, per word": round(
                per_word(name + "_seg_1049x1000", s1000.T) / per_word(name + "_a", W), 4),
        }
        hot[name] = res
    result["hot_path"] = {"words": W, "words_1049x1000": s1000.T, "timing": "kernel dispatch events", **hot}
    del one, s1024, flat

    # the last tile: lane by lane (this library) against the whole tile per character (--variant-lib)
    if a.variant_lib:
        V = C.CDLL(os.path.abspath(a.variant_lib))
        V.amph_last_error.restype = C.c_char_p
        V.amph_build_id.restype = C.c_char_p
        for fn in ("amph_recombine_verify_b64_packed", "amph_mask_input_b64_packed", "amph_ctx_create",
                   "amph_time_next_launch"):
            getattr(V, fn).argtypes = getattr(L, fn).argtypes
        vh = C.c_void_p()
        ok(V.amph_ctx_create(_lib.le16(TEST_PRIME), _lib.le16(TEST_R), _lib.le16(TEST_RINV), 0, C.byref(vh)), V)

        def timed(lib):
            def measure(fn):
                lib.amph_time_next_launch(ev[0].handle, ev[1].handle)
                fn()
                torch.cuda.synchronize()
                return ev[0].elapsed_ms(ev[1])
            return measure

        s100 = Shape(buf, secrets, 10485, 100)
        last = {}
        for sname, sh in (("1000_words", s1000), ("100_words", s100)):
            for seg in ("rv", "mask"):
                rows = {"lanes_a": (L, lambda sh=sh, seg=seg: getattr(sh, seg)()),
                        "tile": (V, lambda sh=sh, seg=seg: getattr(sh, seg)(V, vh)),
                        "lanes_a2": (L, lambda sh=sh, seg=seg: getattr(sh, seg)())}
                ts = {k: [] for k in rows}
                for r in range(a.reps + a.warmup):
                    for k, (lib, fn) in rows.items():
                        t = timed(lib)(fn)
                        if r >= a.warmup:
                            ts[k].append(t)
                res = {k: stats(v) for k, v in ts.items()}
                assert sh.clean()
                res["ratios"] = {"lanes_a2_over_a (spread)": ratio(res, "lanes_a2", "lanes_a"),
                                 "tile_over_lanes": ratio(res, "tile", "lanes_a")}
                last["%s_%s" % (seg, sname)] = res
        result["last_tile"] = {"objects_of_1000_words": s1000.K, "objects_of_100_words": s100.K,
                               "variant_build_id": V.amph_build_id().decode(),
                               "timing": "kernel dispatch events", **last}
        del s100
    del s1000

    # what batching buys: 256 objects x 1,000 words
    K, WO = 256, 1000
    nc, sl, T = nchars_of(WO), slot_of(WO), K * WO
    sh = Shape(buf, secrets, K, WO)
    hbufs = [[sh.bufs[k][j].cpu().numpy() for j in range(N)] for k in range(5)]
    hsec = secrets[:T].cpu().numpy()
    hptr = lambda x: x.ctypes.data  # noqa: E731
    singles_h = [b64_structs(hbufs, nc, o * sl, hptr) for o in range(K)]
    singles_d = [b64_structs(sh.bufs, nc, o * sl) for o in range(K)]
    gathered = (_lib._AmphOdoB64 * (K * N))(*[s[j] for s in singles_h for j in range(N)])
    words = (C.c_size_t * K)(*([WO] * K))
    h16, h24 = np.empty((T, 16), np.uint8), np.empty((T, 24), np.uint8)
    hff, hbad = np.full(K, -1, np.int64), np.full(K, -1, np.int64)
    p16 = (C.c_void_p * K)(*[h16.ctypes.data + 16 * WO * o for o in range(K)])
    p24 = (C.c_void_p * K)(*[h24.ctypes.data + 24 * WO * o for o in range(K)])
    psec = (C.c_void_p * K)(*[hsec.ctypes.data + 16 * WO * o for o in range(K)])
    at = lambda x, o: C.cast(C.c_void_p(x.ctypes.data + 8 * o), i64p)  # noqa: E731
    dat = lambda x, o: C.cast(C.c_void_p(x.data_ptr() + 8 * o), i64p)  # noqa: E731
    # decode-then-packed: 5 n decoded field arrays, then amph_*_packed on them
    dec = np.empty((5, N, T, 16), np.uint8)
    dec_odos = (_lib._AmphOdo * N)(*[_lib._AmphOdo(*[dec[k, j].ctypes.data for k in range(5)], 16 * T)
                                     for j in range(N)])
    offsets = np.arange(0, T + 1, WO, dtype=np.uint64)
    nbytes = C.c_size_t()

    def decode_all():
        for o in range(K):
            for j in range(N):
                for k in range(5):
                    ok(L.amph_base64_decode(ctx._h, hbufs[k][j].ctypes.data + o * sl, nc,
                                            dec[k, j].ctypes.data + 16 * WO * o, C.byref(nbytes), None, 0, None))

    def host_singles(masked):
        for o in range(K):
            if masked:
                ok(L.amph_mask_input_b64(ctx._h, singles_h[o], N, WO, psec[o], WO, p16[o], p24[o], at(hff, o),
                                         at(hbad, o), 0, None))
            else:
                ok(L.amph_recombine_verify_b64(ctx._h, singles_h[o], N, WO, p16[o], at(hff, o), at(hbad, o), 0,
                                               None))

    def dev_singles(masked):
        for o in range(K):
            if masked:
                ok(L.amph_mask_input_b64(ctx._h, singles_d[o], N, WO, sh.sec.data_ptr() + 16 * WO * o, WO,
                                         sh.o16.data_ptr() + 16 * WO * o, sh.o24.data_ptr() + 24 * WO * o,
                                         dat(sh.ff, o), dat(sh.bad, o), F_DEV, stream))
            else:
                ok(L.amph_recombine_verify_b64(ctx._h, singles_d[o], N, WO, sh.o16.data_ptr() + 16 * WO * o,
                                               dat(sh.ff, o), dat(sh.bad, o), F_DEV, stream))
        torch.cuda.synchronize()

    def synced(fn):
        fn()
        torch.cuda.synchronize()

    i64 = lambda x: x.ctypes.data_as(i64p)  # noqa: E731
    breps = max(5, a.reps // 2)
    bat = alternate({
        "host_256_recombine_verify_b64": lambda: host_singles(False),
        "host_recombine_verify_b64_batch": lambda: ok(L.amph_recombine_verify_b64_batch(
            ctx._h, gathered, N, K, words, p16, i64(hff), i64(hbad), 0)),
        "host_decode_then_recombine_verify_packed": lambda: (decode_all(), ok(L.amph_recombine_verify_packed(
            ctx._h, dec_odos, N, offsets.ctypes.data, K, h16.ctypes.data, hff.ctypes.data, 0, None))),
        "host_256_mask_input_b64": lambda: host_singles(True),
        "host_mask_input_b64_batch": lambda: ok(L.amph_mask_input_b64_batch(
            ctx._h, gathered, N, K, words, psec, p16, p24, i64(hff), i64(hbad), 0)),
        "host_decode_then_mask_input_packed": lambda: (decode_all(), ok(L.amph_mask_input_packed(
            ctx._h, dec_odos, N, offsets.ctypes.data, K, hsec.ctypes.data, h16.ctypes.data, hff.ctypes.data, 0,
            None))),
        "device_256_recombine_verify_b64": lambda: dev_singles(False),
        "device_recombine_verify_b64_packed": lambda: synced(sh.rv),
        "device_256_mask_input_b64": lambda: dev_singles(True),
        "device_mask_input_b64_packed": lambda: synced(sh.mask),
    }, breps, 3, wall_ms)
    assert list(hff) == [-1] * K and list(hbad) == [-1] * K and sh.clean()
    bat["speedup"] = {
        "host_recombine_verify_b64: singles / batch": ratio(bat, "host_256_recombine_verify_b64",
                                                            "host_recombine_verify_b64_batch"),
        "host_recombine_verify: decode + packed / batch": ratio(bat, "host_decode_then_recombine_verify_packed",
                                                                "host_recombine_verify_b64_batch"),
        "host_mask_input_b64: singles / batch": ratio(bat, "host_256_mask_input_b64", "host_mask_input_b64_batch"),
        "host_mask_input: decode + packed / batch": ratio(bat, "host_decode_then_mask_input_packed",
                                                          "host_mask_input_b64_batch"),
        "device_recombine_verify_b64: singles / packed": ratio(bat, "device_256_recombine_verify_b64",
                                                               "device_recombine_verify_b64_packed"),
        "device_mask_input_b64: singles / packed": ratio(bat, "device_256_mask_input_b64",
                                                         "device_mask_input_b64_packed"),
    }
    result["batching"] = {"objects": K, "words_per_object": WO, "field_decodes_per_object": 5 * N,
                          "timing": "wall clock, one synchronise per side", "reps": breps, **bat}
    emit(result)


# ---------------------------------------------------------------- --upload
def upload_mode():
    F_DEV = _lib.AMPH_F_DEVICE
    stream = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    nchars_of, slot_of = _lib.wire_text_chars, _lib.wire_slot_chars
    chars_of, stride_of = _lib.masked_input_data_chars, _lib.upload_slot_chars
    NF = _lib.AMPH_NO_FAILURE

    def ok(st):
        if st != 0:
            raise RuntimeError(L.amph_last_error().decode())

    def synced(fn):
        fn()
        torch.cuda.synchronize()

    K, WO = 256, 1000
    T = K * WO
    hptr = lambda x: x.ctypes.data  # noqa: E731
    at = lambda x, o: C.cast(C.c_void_p(x.ctypes.data + 8 * o), i64p)  # noqa: E731
    dat = lambda x, o: C.cast(C.c_void_p(x.data_ptr() + 8 * o), i64p)  # noqa: E731
    i64 = lambda x: x.ctypes.data_as(i64p)  # noqa: E731
    breps = max(5, a.reps // 2)
    secrets = ctx.synth_words(12, T)
    hsec = secrets.cpu().numpy()
    words = (C.c_size_t * K)(*([WO] * K))
    ostride, ochars = stride_of(WO), chars_of(WO)
    result = {"tool": "bench_batch --upload", "build_id": _lib.check_build_id(),
              "device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "objects": K,
              "words_per_object": WO, "batching_reps": breps,
              "timing": {"batching": "wall clock, one synchronise per side", "hot_path": "kernel dispatch events"}}

    # ---- client side: K secrets -> K framed texts, at 2 and 3 parties
    client, texts_dev = {}, None
    for n in (2, 3):
        _, buf, _ = ctx.synth_odos(11, n, T, noncanon_permille=20)  # (5, n, T, 16)
        nc, sl = nchars_of(WO), slot_of(WO)
        bufs = [[slotted(buf[k, j], K, WO) for j in range(n)] for k in range(5)]
        one = [[slotted(buf[k, j], 1, T) for j in range(n)] for k in range(5)]  # ONE object of T words
        del buf
        woff = torch.arange(0, T + 1, WO, dtype=torch.int64, device="cuda")
        toff = torch.arange(0, K * sl, sl, dtype=torch.int64, device="cuda")
        ooff = torch.arange(0, K * ostride, ostride, dtype=torch.int64, device="cuda")
        out_d = torch.zeros(K * ostride, dtype=torch.uint8, device="cuda")
        out_s = torch.zeros(K * ostride, dtype=torch.uint8, device="cuda")
        ff, bad = (torch.empty(K, dtype=torch.int64, device="cuda") for _ in range(2))
        packed = b64_structs(bufs, K * sl, n=n)
        singles_d = [b64_structs(bufs, nc, o * sl, n=n) for o in range(K)]
        hbufs = [[bufs[k][j].cpu().numpy() for j in range(n)] for k in range(5)]
        singles_h = [b64_structs(hbufs, nc, o * sl, hptr, n=n) for o in range(K)]
        gathered = (_lib._AmphOdoB64 * (K * n))(*[s[j] for s in singles_h for j in range(n)])
        hout_b, hout_s = np.zeros(K * ostride, np.uint8), np.zeros(K * ostride, np.uint8)
        hff, hbad = np.full(K, -1, np.int64), np.full(K, -1, np.int64)
        pout_b = (C.c_void_p * K)(*[hout_b.ctypes.data + ostride * o for o in range(K)])
        psec = (C.c_void_p * K)(*[hsec.ctypes.data + 16 * WO * o for o in range(K)])

        def host_singles():
            for o in range(K):
                ok(L.amph_mask_input_json(ctx._h, singles_h[o], n, WO, psec[o], WO, hout_s.ctypes.data + ostride * o,
                                          ochars, at(hff, o), at(hbad, o), 0, None))

        def dev_singles():
            for o in range(K):
                ok(L.amph_mask_input_json(ctx._h, singles_d[o], n, WO, secrets.data_ptr() + 16 * WO * o, WO,
                                          out_s.data_ptr() + ostride * o, ochars, dat(ff, o), dat(bad, o), F_DEV,
                                          stream))
            torch.cuda.synchronize()

        def dev_packed():
            ok(L.amph_mask_input_json_packed(ctx._h, packed, n, woff.data_ptr(), toff.data_ptr(), K,
                                             secrets.data_ptr(), out_d.data_ptr(), K * ostride, ooff.data_ptr(),
                                             ff.data_ptr(), bad.data_ptr(), F_DEV, stream))

        bat = alternate({
            "host_256_mask_input_json": host_singles,
            "host_mask_input_json_batch": lambda: ok(L.amph_mask_input_json_batch(
                ctx._h, gathered, n, K, words, psec, pout_b, i64(hff), i64(hbad), 0)),
            "device_256_mask_input_json": dev_singles,
            "device_mask_input_json_packed": lambda: synced(dev_packed),
        }, breps, 3, wall_ms)
        assert list(hff) == [-1] * K and list(hbad) == [-1] * K and bool((ff == NF).all()) and bool((bad == NF).all())
        assert np.array_equal(hout_b, hout_s) and torch.equal(out_d, out_s) and np.array_equal(out_d.cpu().numpy(), hout_b)
        bat["speedup"] = {
            "host: singles / batch": ratio(bat, "host_256_mask_input_json", "host_mask_input_json_batch"),
            "device: singles / packed": ratio(bat, "device_256_mask_input_json", "device_mask_input_json_packed"),
        }
        # hot path: one object of T words, the single call's own text and layout
        flat = b64_structs(one, nchars_of(T), n=n)
        w1 = torch.tensor([0, T], dtype=torch.int64, device="cuda")
        z1 = torch.zeros(1, dtype=torch.int64, device="cuda")
        t_flat = torch.zeros(stride_of(T), dtype=torch.uint8, device="cuda")
        t_seg = torch.zeros(stride_of(T), dtype=torch.uint8, device="cuda")
        ff1, bad1 = (torch.empty(1, dtype=torch.int64, device="cuda") for _ in range(2))

        def k_flat():
            ok(L.amph_mask_input_json(ctx._h, flat, n, T, secrets.data_ptr(), T, t_flat.data_ptr(), chars_of(T),
                                      dat(ff1, 0), dat(bad1, 0), F_DEV, stream))

        def k_seg():
            ok(L.amph_mask_input_json_packed(ctx._h, flat, n, w1.data_ptr(), z1.data_ptr(), 1, secrets.data_ptr(),
                                             t_seg.data_ptr(), stride_of(T), z1.data_ptr(), ff1.data_ptr(),
                                             bad1.data_ptr(), F_DEV, stream))

        hot = alternate({"k_mask_json_a": k_flat, "k_mask_json_seg_1_object": k_seg, "k_mask_json_a2": k_flat},
                        a.reps, a.warmup, kernel_ms)
        assert torch.equal(t_flat, t_seg) and int(ff1.item()) == NF and int(bad1.item()) == NF
        hot["ratios"] = {"k_mask_json_a2_over_a (spread)": ratio(hot, "k_mask_json_a2", "k_mask_json_a"),
                         "k_mask_json_seg_1_object_over_k_mask_json": ratio(hot, "k_mask_json_seg_1_object",
                                                                            "k_mask_json_a")}
        client["%d_parties" % n] = {"batching": bat, "hot_path_one_object_of_%d_words" % T: hot}
        if n == 2:
            texts_dev, ooff_dev, text_one = out_d, ooff, t_flat[:chars_of(T)]
        del bufs, one, hbufs
    result["client"] = client

    # ---- party side: the K texts the client wrote -> K shares
    tup = ctx.synth_words(13, 2 * T).reshape(T, 32)
    htup, htexts = tup.cpu().numpy(), texts_dev.cpu().numpy()
    key = _lib.le16(123456789)
    woff = torch.arange(0, T + 1, WO, dtype=torch.int64, device="cuda")
    sh_d, sh_s = (torch.zeros((T, 32), dtype=torch.uint8, device="cuda") for _ in range(2))
    bad = torch.empty(K, dtype=torch.int64, device="cuda")
    hsh_b, hsh_s = np.zeros((T, 32), np.uint8), np.zeros((T, 32), np.uint8)
    hbad = np.full(K, -1, np.int64)
    ptxt = (C.c_void_p * K)(*[htexts.ctypes.data + ostride * o for o in range(K)])
    ptup = (C.c_void_p * K)(*[htup.ctypes.data + 32 * WO * o for o in range(K)])
    pout = (C.c_void_p * K)(*[hsh_b.ctypes.data + 32 * WO * o for o in range(K)])
    lens = (C.c_size_t * K)(*([ochars] * K))

    def host_singles():
        for o in range(K):
            ok(L.amph_convert_share_json(ctx._h, ptxt[o], ochars, WO, ptup[o], key, 0,
                                         hsh_s.ctypes.data + 32 * WO * o, at(hbad, o), 0, None))

    def dev_singles():
        for o in range(K):
            ok(L.amph_convert_share_json(ctx._h, texts_dev.data_ptr() + ostride * o, ochars, WO,
                                         tup.data_ptr() + 32 * WO * o, key, 0, sh_s.data_ptr() + 32 * WO * o,
                                         dat(bad, o), F_DEV, stream))
        torch.cuda.synchronize()

    def dev_packed():
        ok(L.amph_convert_share_json_packed(ctx._h, texts_dev.data_ptr(), K * ostride, woff.data_ptr(),
                                            ooff_dev.data_ptr(), K, tup.data_ptr(), key, 0, sh_d.data_ptr(),
                                            bad.data_ptr(), F_DEV, stream))

    bat = alternate({
        "host_256_convert_share_json": host_singles,
        "host_convert_share_json_batch": lambda: ok(L.amph_convert_share_json_batch(
            ctx._h, ptxt, lens, words, K, ptup, key, 0, pout, i64(hbad), 0)),
        "device_256_convert_share_json": dev_singles,
        "device_convert_share_json_packed": lambda: synced(dev_packed),
    }, breps, 3, wall_ms)
    assert list(hbad) == [-1] * K and bool((bad == NF).all())
    assert np.array_equal(hsh_b, hsh_s) and torch.equal(sh_d, sh_s) and np.array_equal(sh_d.cpu().numpy(), hsh_b)
    bat["speedup"] = {
        "host: singles / batch": ratio(bat, "host_256_convert_share_json", "host_convert_share_json_batch"),
        "device: singles / packed": ratio(bat, "device_256_convert_share_json", "device_convert_share_json_packed"),
    }
    w1 = torch.tensor([0, T], dtype=torch.int64, device="cuda")
    z1 = torch.zeros(1, dtype=torch.int64, device="cuda")
    bad1 = torch.empty(1, dtype=torch.int64, device="cuda")

    def k_flat():
        ok(L.amph_convert_share_json(ctx._h, text_one.data_ptr(), chars_of(T), T, tup.data_ptr(), key, 0,
                                     sh_s.data_ptr(), dat(bad1, 0), F_DEV, stream))

    def k_seg():
        ok(L.amph_convert_share_json_packed(ctx._h, text_one.data_ptr(), chars_of(T), w1.data_ptr(), z1.data_ptr(), 1,
                                            tup.data_ptr(), key, 0, sh_d.data_ptr(), bad1.data_ptr(), F_DEV, stream))

    hot = alternate({"k_conv_json_a": k_flat, "k_conv_json_seg_1_object": k_seg, "k_conv_json_a2": k_flat},
                    a.reps, a.warmup, kernel_ms)
    assert torch.equal(sh_d, sh_s) and int(bad1.item()) == NF
    hot["ratios"] = {"k_conv_json_a2_over_a (spread)": ratio(hot, "k_conv_json_a2", "k_conv_json_a"),
                     "k_conv_json_seg_1_object_over_k_conv_json": ratio(hot, "k_conv_json_seg_1_object",
                                                                        "k_conv_json_a")}
    result["party"] = {"batching": bat, "hot_path_one_object_of_%d_words" % T: hot}
    emit(result)


# ---------------------------------------------------------------- --respond
def board_identity():
    """The host and the board's own sysfs identity, as bench.py records them."""
    import socket
    p = torch.cuda.get_device_properties(0)
    bus = "%04x:%02x:%02x.0" % (p.pci_domain_id, p.pci_bus_id, p.pci_device_id)
    out = {"host": socket.gethostname(), "pci_bus_id": bus}
    for k in ("unique_id", "serial_number", "vbios_version", "product_name"):
        try:
            v = open("/sys/bus/pci/devices/%s/%s" % (bus, k)).read().strip()
            if v:
                out[k] = v
        except OSError:
            pass
    return out


def respond_mode():
    F_DEV = _lib.AMPH_F_DEVICE
    stream = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    nchars_of, slot_of = _lib.wire_text_chars, _lib.wire_slot_chars

    def ok(st):
        if st != 0:
            raise RuntimeError(L.amph_last_error().decode())

    K, WO = 256, 1000
    T = K * WO
    sl = slot_of(WO)
    assert nchars_of(WO) <= sl
    breps = max(5, a.reps // 2)
    fields = ctx.synth_words(31, 5 * T).reshape(5, T, 16)
    hfields = fields.cpu().numpy()
    result = {"tool": "bench_batch --respond", "build_id": _lib.check_build_id(),
              "device": torch.cuda.get_device_name(0), "board": board_identity(), "reps": a.reps,
              "warmup": a.warmup, "objects": K, "words_per_object": WO, "batching_reps": breps,
              "timing": {"batching": "wall clock, one synchronise per side", "hot_path": "kernel dispatch events"}}

    # ---- batching: K objects' 5 K texts
    woff = torch.arange(0, T + 1, WO, dtype=torch.int64, device="cuda")
    toff = torch.arange(0, K * sl, sl, dtype=torch.int64, device="cuda")
    out_p = torch.zeros((5, K * sl), dtype=torch.uint8, device="cuda")
    out_s = torch.zeros((5, K * sl), dtype=torch.uint8, device="cuda")
    odo_d = _lib._AmphOdo(*[fields[k].data_ptr() for k in range(5)], 16 * T)
    ob_d = _lib._AmphOdoB64Out(*[out_p[k].data_ptr() for k in range(5)], K * sl)
    hwoff, htoff = woff.cpu().numpy().astype(np.uint64), toff.cpu().numpy().astype(np.uint64)
    hout_p, hout_s, hout_b = (np.zeros((5, K * sl), np.uint8) for _ in range(3))
    odo_h = _lib._AmphOdo(*[hfields[k].ctypes.data for k in range(5)], 16 * T)
    ob_h = _lib._AmphOdoB64Out(*[hout_p[k].ctypes.data for k in range(5)], K * sl)
    gathered = (_lib._AmphOdo * K)(*[_lib._AmphOdo(*[hfields[k].ctypes.data + 16 * WO * o for k in range(5)], 16 * WO)
                                     for o in range(K)])
    pout = (C.c_void_p * (5 * K))(*[hout_b[k].ctypes.data + sl * o for o in range(K) for k in range(5)])
    dsingles = [(fields[k].data_ptr() + 16 * WO * o, out_s[k].data_ptr() + sl * o) for o in range(K) for k in range(5)]
    hsingles = [(hfields[k].ctypes.data + 16 * WO * o, hout_s[k].ctypes.data + sl * o)
                for o in range(K) for k in range(5)]

    def dev_singles():
        for src, dst in dsingles:
            ok(L.amph_base64_encode(ctx._h, src, 16 * WO, dst, F_DEV, stream))
        torch.cuda.synchronize()

    def dev_packed(ob=ob_d, wo=woff, to=toff, k=K):
        ok(L.amph_odo_fields_b64_packed(ctx._h, C.byref(odo_d), wo.data_ptr(), to.data_ptr(), k, C.byref(ob), None,
                                        F_DEV, stream))

    def dev_packed_synced():
        dev_packed()
        torch.cuda.synchronize()

    def host_singles():
        for src, dst in hsingles:
            ok(L.amph_base64_encode(ctx._h, src, 16 * WO, dst, 0, None))

    bat = alternate({
        "device_1280_base64_encode": dev_singles,
        "device_odo_fields_b64_packed": dev_packed_synced,
        "host_1280_base64_encode": host_singles,
        "host_odo_fields_b64_batch": lambda: ok(L.amph_odo_fields_b64_batch(ctx._h, gathered, K, pout, None, 0)),
        "host_odo_fields_b64_packed": lambda: ok(L.amph_odo_fields_b64_packed(
            ctx._h, C.byref(odo_h), hwoff.ctypes.data, htoff.ctypes.data, K, C.byref(ob_h), None, 0, None)),
    }, breps, 3, wall_ms)
    assert torch.equal(out_p, out_s) and np.array_equal(hout_p, hout_s) and np.array_equal(hout_b, hout_s)
    assert np.array_equal(out_p.cpu().numpy(), hout_s)
    d1, dp = bat["device_1280_base64_encode"], bat["device_odo_fields_b64_packed"]
    bat["speedup"] = {
        "device: singles / packed": ratio(bat, "device_1280_base64_encode", "device_odo_fields_b64_packed"),
        "host: singles / batch": ratio(bat, "host_1280_base64_encode", "host_odo_fields_b64_batch"),
        "host: singles / packed": ratio(bat, "host_1280_base64_encode", "host_odo_fields_b64_packed"),
    }
    bat["device_quartile_ranges_disjoint"] = bool(dp["p75_ms"] < d1["p25_ms"])
    result["batching"] = bat

    # ---- hot path: ONE object of T words
    one_chars = slot_of(T)
    o_seg = torch.zeros((5, one_chars), dtype=torch.uint8, device="cuda")
    o_blk = torch.zeros((5, one_chars), dtype=torch.uint8, device="cuda")
    w1 = torch.tensor([0, T], dtype=torch.int64, device="cuda")
    z1 = torch.zeros(1, dtype=torch.int64, device="cuda")
    ob_1 = _lib._AmphOdoB64Out(*[o_seg[k].data_ptr() for k in range(5)], one_chars)

    def five_blk_ms():
        """The five fields' k_b64_encode_blk launches, each timed by its own dispatch events, summed."""
        return sum(kernel_ms(lambda k=k: ok(L.amph_base64_encode(ctx._h, fields[k].data_ptr(), 16 * T,
                                                                 o_blk[k].data_ptr(), F_DEV, stream)))
                   for k in range(5))

    def seg_ms():
        return kernel_ms(lambda: dev_packed(ob=ob_1, wo=w1, to=z1, k=1))

    hot = alternate({"five_k_b64_encode_blk_a": five_blk_ms, "k_odo_b64_seg_1_object": seg_ms,
                     "five_k_b64_encode_blk_a2": five_blk_ms}, a.reps, a.warmup, lambda fn: fn())
    assert torch.equal(o_seg, o_blk)
    base, seg = hot["five_k_b64_encode_blk_a"]["median_ms"], hot["k_odo_b64_seg_1_object"]["median_ms"]
    hot["ratios"] = {"five_blk_a2_over_a (spread)": ratio(hot, "five_k_b64_encode_blk_a2", "five_k_b64_encode_blk_a"),
                     "k_odo_b64_seg_1_object_over_five_blk": ratio(hot, "k_odo_b64_seg_1_object",
                                                                   "five_k_b64_encode_blk_a")}
    hot["difference_us"] = {"seg_minus_five_blk": round(1e3 * (seg - base), 3),
                            "five_blk_a2_minus_a (spread)": round(
                                1e3 * (hot["five_k_b64_encode_blk_a2"]["median_ms"] - base), 3)}
    result["hot_path_one_object_of_%d_words" % T] = hot

    emit(result)


# ---------------------------------------------------------------- --exchange
def exchange_mode():
    """256 objects x 2,000 pairs of full-length diffs, 3 parties' worth of
    texts per round (one encode, two partners' decodes): the batch calls
    against 256 (+ 512) single calls, device and host mode, wall clock with one
    synchronise per side.  Then ONE object of 512,000 pairs: the batch call's
    kernel time against the single call's, rows a / batch / a2 alternating."""
    F_DEV = _lib.AMPH_F_DEVICE
    stream = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)

    def ok(st):
        if st != 0:
            raise RuntimeError(L.amph_last_error().decode())

    def diffs(seed, pairs):
        mag = ctx.synth_words(seed, 2 * pairs).reshape(pairs, 2, 16)  # field elements: 38-39 digits each
        neg = (ctx.synth_words(seed + 1, (2 * pairs + 15) // 16).reshape(-1)[:2 * pairs] & 1).reshape(pairs, 2)
        return mag.contiguous(), neg.contiguous()

    K, PO, PARTNERS = 256, 2000, 2
    T = K * PO
    sl, mx = _lib.exchange_slot_chars(PO), int(L.amph_exchange_max_chars(PO))
    breps = max(5, a.reps // 2)
    result = {"tool": "bench_batch --exchange", "build_id": _lib.check_build_id(),
              "device": torch.cuda.get_device_name(0), "board": board_identity(), "reps": a.reps,
              "warmup": a.warmup, "objects": K, "pairs_per_object": PO, "partner_texts_per_object": PARTNERS,
              "batching_reps": breps,
              "timing": {"batching": "wall clock, one synchronise per side", "hot_path": "kernel dispatch events"}}
    mag, neg = diffs(41, T)
    hmag, hneg = mag.cpu().numpy(), neg.cpu().numpy()
    poff = torch.arange(0, T + 1, PO, dtype=torch.int64, device="cuda")
    toff = torch.arange(0, K * sl, sl, dtype=torch.int64, device="cuda")
    hpoff, htoff = poff.cpu().numpy().astype(np.uint64), toff.cpu().numpy().astype(np.uint64)
    text_p = torch.zeros(K * sl, dtype=torch.uint8, device="cuda")
    text_s = torch.zeros(K * sl, dtype=torch.uint8, device="cuda")
    lens_p = torch.zeros(K, dtype=torch.int64, device="cuda")
    lens_s = torch.zeros(K, dtype=torch.int64, device="cuda")
    omag_p, omag_s = torch.zeros_like(mag), torch.zeros_like(mag)
    oneg_p, oneg_s = torch.zeros_like(neg), torch.zeros_like(neg)
    bad_p = torch.zeros(K, dtype=torch.int64, device="cuda")
    bad_s = torch.zeros(K, dtype=torch.int64, device="cuda")
    htext_p, htext_s = np.zeros(K * sl, np.uint8), np.zeros(K * sl, np.uint8)
    hlens_p, hlens_s = np.zeros(K, np.uint64), np.zeros(K, np.uint64)
    homag_p, homag_s = np.zeros_like(hmag), np.zeros_like(hmag)
    honeg_p, honeg_s = np.zeros_like(hneg), np.zeros_like(hneg)
    hbad_p, hbad_s = np.zeros(K, np.int64), np.zeros(K, np.int64)
    hl = []  # the texts' lengths on the host, once the first encode has run

    def dev_packed():
        ok(L.amph_exchange_encode_packed(ctx._h, mag.data_ptr(), neg.data_ptr(), T, poff.data_ptr(), toff.data_ptr(),
                                         K, text_p.data_ptr(), K * sl, lens_p.data_ptr(), F_DEV, stream))
        for _ in range(PARTNERS):
            ok(L.amph_exchange_decode_packed(ctx._h, text_p.data_ptr(), K * sl, poff.data_ptr(), toff.data_ptr(),
                                             lens_p.data_ptr(), K, T, omag_p.data_ptr(), oneg_p.data_ptr(),
                                             C.cast(C.c_void_p(bad_p.data_ptr()), i64p), F_DEV, stream))
        torch.cuda.synchronize()

    def dev_singles():
        for o in range(K):
            ok(L.amph_exchange_encode(ctx._h, mag.data_ptr() + 32 * PO * o, neg.data_ptr() + 2 * PO * o, PO,
                                      text_s.data_ptr() + sl * o, mx, lens_s.data_ptr() + 8 * o, F_DEV, stream))
        for _ in range(PARTNERS):
            for o in range(K):
                ok(L.amph_exchange_decode(ctx._h, text_s.data_ptr() + sl * o, hl[o], PO,
                                          omag_s.data_ptr() + 32 * PO * o, oneg_s.data_ptr() + 2 * PO * o,
                                          C.cast(C.c_void_p(bad_s.data_ptr() + 8 * o), i64p), F_DEV, stream))
        torch.cuda.synchronize()

    def host_packed():
        ok(L.amph_exchange_encode_packed(ctx._h, hmag.ctypes.data, hneg.ctypes.data, T, hpoff.ctypes.data,
                                         htoff.ctypes.data, K, htext_p.ctypes.data, K * sl, hlens_p.ctypes.data, 0,
                                         None))
        for _ in range(PARTNERS):
            ok(L.amph_exchange_decode_packed(ctx._h, htext_p.ctypes.data, K * sl, hpoff.ctypes.data,
                                             htoff.ctypes.data, hlens_p.ctypes.data, K, T, homag_p.ctypes.data,
                                             honeg_p.ctypes.data, hbad_p.ctypes.data_as(i64p), 0, None))

    def host_singles():
        for o in range(K):
            ok(L.amph_exchange_encode(ctx._h, hmag.ctypes.data + 32 * PO * o, hneg.ctypes.data + 2 * PO * o, PO,
                                      htext_s.ctypes.data + sl * o, mx, hlens_s.ctypes.data + 8 * o, 0, None))
        for _ in range(PARTNERS):
            for o in range(K):
                ok(L.amph_exchange_decode(ctx._h, htext_s.ctypes.data + sl * o, int(hlens_s[o]), PO,
                                          homag_s.ctypes.data + 32 * PO * o, honeg_s.ctypes.data + 2 * PO * o,
                                          hbad_s[o:].ctypes.data_as(i64p), 0, None))

    dev_packed()
    hl.extend(int(x) for x in lens_p.cpu().numpy())
    names = ["device_%d_single_calls" % (K * (1 + PARTNERS)), "device_packed_calls",
             "host_%d_single_calls" % (K * (1 + PARTNERS)), "host_packed_calls"]
    bat = alternate(dict(zip(names, (dev_singles, dev_packed, host_singles, host_packed))), breps, 3, wall_ms)
    NFV = 0x7F7F7F7F7F7F7F7F
    assert torch.equal(lens_p, lens_s) and torch.equal(omag_p, omag_s) and torch.equal(oneg_p, oneg_s)
    assert bool((bad_p == NFV).all()) and bool((bad_s == NFV).all())
    tp, ts = text_p.cpu().numpy(), text_s.cpu().numpy()
    for o in range(K):
        lo, hi = sl * o, sl * o + hl[o]
        assert np.array_equal(tp[lo:hi], ts[lo:hi]) and np.array_equal(htext_p[lo:hi], ts[lo:hi])
    assert np.array_equal(omag_p.cpu().numpy(), hmag) and np.array_equal(homag_p, hmag) and np.array_equal(homag_s, hmag)
    assert (hbad_p == -1).all() and (hbad_s == -1).all() and np.array_equal(hlens_p, hlens_s)
    bat["speedup"] = {"device: singles / packed": ratio(bat, names[0], names[1]),
                      "host: singles / packed": ratio(bat, names[2], names[3])}
    bat["device_quartile_ranges_disjoint"] = bool(bat[names[1]]["p75_ms"] < bat[names[0]]["p25_ms"])
    bat["host_quartile_ranges_disjoint"] = bool(bat[names[3]]["p75_ms"] < bat[names[2]]["p25_ms"])
    result["batching"] = bat

    # ---- hot path: ONE object of 512,000 pairs, kernel time of the whole call (first launch to last)
    P1 = 512000
    m1, g1 = diffs(51, P1)
    cap1 = _lib.exchange_slot_chars(P1)
    t_seg = torch.zeros(cap1, dtype=torch.uint8, device="cuda")
    t_one = torch.zeros(cap1, dtype=torch.uint8, device="cuda")
    p1 = torch.tensor([0, P1], dtype=torch.int64, device="cuda")
    z1 = torch.zeros(1, dtype=torch.int64, device="cuda")
    l_seg, l_one = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    om_seg, om_one = torch.zeros_like(m1), torch.zeros_like(m1)
    on_seg, on_one = torch.zeros_like(g1), torch.zeros_like(g1)
    b_seg, b_one = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")

    def enc_one():
        ok(L.amph_exchange_encode(ctx._h, m1.data_ptr(), g1.data_ptr(), P1, t_one.data_ptr(), cap1, l_one.data_ptr(),
                                  F_DEV, stream))

    def enc_seg():
        ok(L.amph_exchange_encode_packed(ctx._h, m1.data_ptr(), g1.data_ptr(), P1, p1.data_ptr(), z1.data_ptr(), 1,
                                         t_seg.data_ptr(), cap1, l_seg.data_ptr(), F_DEV, stream))
    enc_one()
    enc_seg()
    torch.cuda.synchronize()
    n1 = int(l_one.item())
    assert n1 == int(l_seg.item()) and torch.equal(t_one[:n1], t_seg[:n1])

    def dec_one():
        ok(L.amph_exchange_decode(ctx._h, t_one.data_ptr(), n1, P1, om_one.data_ptr(), on_one.data_ptr(),
                                  C.cast(C.c_void_p(b_one.data_ptr()), i64p), F_DEV, stream))

    def dec_seg():
        ok(L.amph_exchange_decode_packed(ctx._h, t_seg.data_ptr(), cap1, p1.data_ptr(), z1.data_ptr(),
                                         l_seg.data_ptr(), 1, P1, om_seg.data_ptr(), on_seg.data_ptr(),
                                         C.cast(C.c_void_p(b_seg.data_ptr()), i64p), F_DEV, stream))
    rows = {"exchange_encode_a": enc_one, "exchange_encode_packed_1_object": enc_seg, "exchange_encode_a2": enc_one,
            "exchange_decode_a": dec_one, "exchange_decode_packed_1_object": dec_seg, "exchange_decode_a2": dec_one}
    hot = alternate(rows, a.reps, a.warmup, kernel_ms)
    assert torch.equal(om_one, om_seg) and torch.equal(on_one, on_seg) and torch.equal(om_one, m1)
    assert int(b_one.item()) == NFV and int(b_seg.item()) == NFV
    hot["difference_us"] = {}
    for k in ("encode", "decode"):
        base = hot["exchange_%s_a" % k]["median_ms"]
        hot["difference_us"]["%s: packed minus single" % k] = round(
            1e3 * (hot["exchange_%s_packed_1_object" % k]["median_ms"] - base), 3)
        hot["difference_us"]["%s: single a2 minus a (spread)" % k] = round(
            1e3 * (hot["exchange_%s_a2" % k]["median_ms"] - base), 3)
    hot["text_chars"] = n1
    result["hot_path_one_object_of_%d_pairs" % P1] = hot
    emit(result)


def exchange_single_mode():
    """--exchange-single --parent-lib LIB [--parent-lib-copy LIB2]: the SINGLE
    calls amph_exchange_encode / amph_exchange_decode at 8 Mi pairs, this
    tree's library against another build's (the parent commit's, built from a
    checkout of it) loaded beside it in this process.  Kernel time of the whole
    call; every row takes every place in the round in turn; the other build
    twice per round (a, a2: its own spread) and, with --parent-lib-copy, a
    byte-for-byte copy of it under another path loaded a third time: what two
    loads of the same code differ by (their own contexts and scratch)."""
    if not a.parent_lib:
        sys.exit("--exchange-single needs --parent-lib")
    vp, sz, i32, u32 = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32

    def load(path):
        lib = C.CDLL(os.path.abspath(path))
        lib.amph_ctx_create.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, i32, C.POINTER(vp)]
        lib.amph_ctx_destroy.argtypes = [vp]
        lib.amph_exchange_encode.argtypes = [vp, vp, vp, sz, vp, sz, vp, u32, vp]
        lib.amph_exchange_decode.argtypes = [vp, vp, sz, sz, vp, vp, i64p, u32, vp]
        lib.amph_time_next_launch.argtypes = [vp, vp]
        lib.amph_timing_event_create.argtypes = [C.POINTER(vp)]
        lib.amph_timing_event_elapsed_ms.argtypes = [vp, vp, C.POINTER(C.c_float)]
        lib.amph_build_id.restype = C.c_char_p
        lib.amph_last_error.restype = C.c_char_p
        h = vp()
        keys = [_lib.le16(x) for x in (TEST_PRIME, TEST_R, TEST_RINV)]
        assert lib.amph_ctx_create(*keys, 0, C.byref(h)) == 0, lib.amph_last_error()
        return lib, h

    def events(lib):
        e0, e1 = vp(), vp()
        assert lib.amph_timing_event_create(C.byref(e0)) == 0 and lib.amph_timing_event_create(C.byref(e1)) == 0
        return e0, e1

    builds = {"this tree": (L, ctx._h, events(L))}
    lib, h = load(a.parent_lib)
    builds["parent"] = (lib, h, events(lib))
    parent_id = lib.amph_build_id().decode()
    if a.parent_lib_copy:
        lib, h = load(a.parent_lib_copy)
        assert lib.amph_build_id().decode() == parent_id, "--parent-lib-copy must be the same build"
        builds["parent, second load"] = (lib, h, events(lib))
    stream = vp(torch.cuda.current_stream(0).cuda_stream)
    P = 8 << 20
    mag = ctx.synth_words(61, 2 * P).reshape(P, 2, 16).contiguous()
    neg = (ctx.synth_words(62, (2 * P + 15) // 16).reshape(-1)[:2 * P] & 1).reshape(P, 2).contiguous()
    cap = int(L.amph_exchange_max_chars(P))
    text = {k: torch.zeros(cap, dtype=torch.uint8, device="cuda") for k in builds}
    ln = {k: torch.zeros(1, dtype=torch.int64, device="cuda") for k in builds}
    om, on = torch.zeros_like(mag), torch.zeros_like(neg)
    bad = torch.zeros(1, dtype=torch.int64, device="cuda")

    def timed(which, fn):
        lib, h, (e0, e1) = builds[which]
        lib.amph_time_next_launch(e0, e1)
        assert fn(lib, h) == 0, lib.amph_last_error()
        torch.cuda.synchronize()
        ms = C.c_float()
        assert lib.amph_timing_event_elapsed_ms(e0, e1, C.byref(ms)) == 0
        return ms.value

    def enc(which):
        return timed(which, lambda lib, h: lib.amph_exchange_encode(
            h, mag.data_ptr(), neg.data_ptr(), P, text[which].data_ptr(), cap, ln[which].data_ptr(),
            _lib.AMPH_F_DEVICE, stream))

    for k in builds:
        enc(k)
    n = int(ln["this tree"].item())
    for k in builds:
        assert int(ln[k].item()) == n and torch.equal(text[k][:n], text["this tree"][:n]), k

    def dec(which):
        return timed(which, lambda lib, h: lib.amph_exchange_decode(
            h, text["this tree"].data_ptr(), n, P, om.data_ptr(), on.data_ptr(), C.cast(vp(bad.data_ptr()), i64p),
            _lib.AMPH_F_DEVICE, stream))

    order = ["parent a", "this tree", "parent a2"] + (["parent, second load"] if a.parent_lib_copy else [])
    build_of = {"parent a": "parent", "parent a2": "parent"}
    ts = {"%s %s" % (op, k): [] for op in ("encode", "decode") for k in order}
    for r in range(a.reps + a.warmup):
        rot = r % len(order)
        for op, fn in (("encode", enc), ("decode", dec)):
            for k in order[rot:] + order[:rot]:
                t = fn(build_of.get(k, k))
                if r >= a.warmup:
                    ts["%s %s" % (op, k)].append(t)
    assert torch.equal(om, mag) and int(bad.item()) == 0x7F7F7F7F7F7F7F7F
    result = {"tool": "bench_batch --exchange-single", "pairs": P, "text_chars": n, "reps": a.reps,
              "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "board": board_identity(),
              "parent_build_id": parent_id, "build_id": _lib.check_build_id(),
              "timing": "kernel dispatch events, first launch of the call to its last",
              "rows": {k: stats(v) for k, v in ts.items()}}
    for op in ("encode", "decode"):
        base = result["rows"]["%s parent a" % op]["median_ms"]
        result["%s_us" % op] = {"%s minus parent a" % k: round(
            1e3 * (result["rows"]["%s %s" % (op, k)]["median_ms"] - base), 3) for k in order[1:]}
    emit(result)


if a.exchange_single:
    exchange_single_mode()
    del ctx  # (destroyed while the library is still loaded)
    sys.exit(0)

if a.exchange:
    exchange_mode()
    del ctx  # (destroyed while the library is still loaded)
    sys.exit(0)

if a.respond:
    respond_mode()
    del ctx  # (destroyed while the library is still loaded)
    sys.exit(0)

if a.upload:
    upload_mode()
    del ctx  # (destroyed while the library is still loaded)
    sys.exit(0)

if a.wire:
    wire_mode()
    del ctx  # (destroyed while the library is still loaded)
    sys.exit(0)


# ---------------------------------------------------------------- hot path
W = 1 << 20
odos, buf, _ = ctx.synth_odos(11, N, W, noncanon_permille=20)
secrets = ctx.synth_words(12, W)
out = torch.empty((W, 16), dtype=torch.uint8, device="cuda")
one = torch.tensor([0, W], dtype=torch.int64, device="cuda")
many = torch.arange(0, W + 1, 1024, dtype=torch.int64, device="cuda")
ff1 = torch.empty(1, dtype=torch.int64, device="cuda")
ffk = torch.empty(many.numel() - 1, dtype=torch.int64, device="cuda")


def hot(bodos):
    rv = alternate({
        "k_rv_a": lambda: ctx.recombine_verify(bodos, out=out),
        "k_rv_seg_1_object": lambda: ctx.recombine_verify_packed(bodos, one, out=out, first_fail=ff1),
        "k_rv_seg_1024_objects": lambda: ctx.recombine_verify_packed(bodos, many, out=out, first_fail=ffk),
        "k_rv_a2": lambda: ctx.recombine_verify(bodos, out=out),
    }, a.reps, a.warmup, kernel_ms)
    mk = alternate({
        "k_mask_a": lambda: ctx.mask_input(bodos, secrets, out=out),
        "k_mask_seg_1_object": lambda: ctx.mask_input_packed(bodos, one, secrets, out=out, first_fail=ff1),
        "k_mask_seg_1024_objects": lambda: ctx.mask_input_packed(bodos, many, secrets, out=out, first_fail=ffk),
        "k_mask_a2": lambda: ctx.mask_input(bodos, secrets, out=out),
    }, a.reps, a.warmup, kernel_ms)
    res = {**rv, **mk}
    res["ratios"] = {
        "k_rv_a2_over_a (spread)": ratio(res, "k_rv_a2", "k_rv_a"),
        "k_rv_seg_1_object_over_k_rv": ratio(res, "k_rv_seg_1_object", "k_rv_a"),
        "k_rv_seg_1024_objects_over_k_rv": ratio(res, "k_rv_seg_1024_objects", "k_rv_a"),
        "k_mask_a2_over_a (spread)": ratio(res, "k_mask_a2", "k_mask_a"),
        "k_mask_seg_1_object_over_k_mask": ratio(res, "k_mask_seg_1_object", "k_mask_a"),
        "k_mask_seg_1024_objects_over_k_mask": ratio(res, "k_mask_seg_1024_objects", "k_mask_a"),
    }
    return res


result = {"tool": "bench_batch", "build_id": _lib.check_build_id(), "device": torch.cuda.get_device_name(0),
          "parties": N, "reps": a.reps, "warmup": a.warmup}
result["hot_path"] = {"words": W, "timing": "kernel dispatch events", **hot(odos)}
assert int(ff1.item()) == _lib.AMPH_NO_FAILURE and bool((ffk == _lib.AMPH_NO_FAILURE).all())

# worst case: every word fails (<w> of party 0 off by one everywhere)
bad = buf.clone()
bad[3, 0, :, 0] ^= 1
bad_odos = [tuple(bad[k, j] for k in range(5)) for j in range(N)]
result["every_word_fails"] = {"words": W, "timing": "kernel dispatch events", **hot(bad_odos)}
assert int(ff1.item()) == 0 and bool((ffk == 0).all())
del bad, bad_odos

# ---------------------------------------------------------------- batching
K, WO = 256, 1000
T = K * WO
bodos, bbuf, _ = ctx.synth_odos(21, N, T, noncanon_permille=20)
bsec = ctx.synth_words(22, T)
hbuf = bbuf.cpu().numpy()  # (5, N, T, 16)
hsec = bsec.cpu().numpy()
offsets = np.arange(0, T + 1, WO, dtype=np.uint64)
doff = torch.from_numpy(offsets.view(np.int64)).cuda()
torch.cuda.synchronize()
stream = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
F_DEV = _lib.AMPH_F_DEVICE


def odo_struct(base, j, lo, words, ptr):
    return _lib._AmphOdo(*[ptr(base[k, j]) + 16 * lo for k in range(5)], 16 * words)


def host_ptr(x):
    return x.ctypes.data


def dev_ptr(x):
    return x.data_ptr()


# host mode: K singles over slices of the packed arrays against one gathered call
hout = np.empty((T, 16), np.uint8)
hff = np.full(K, -1, np.int64)
singles = []
for o in range(K):
    arr = (_lib._AmphOdo * N)(*[odo_struct(hbuf, j, o * WO, WO, host_ptr) for j in range(N)])
    singles.append((arr, hout.ctypes.data + 16 * o * WO, hsec.ctypes.data + 16 * o * WO,
                    C.cast(C.c_void_p(hff.ctypes.data + 8 * o), i64p)))
gathered = (_lib._AmphOdo * (K * N))(*[odo_struct(hbuf, j, o * WO, WO, host_ptr) for o in range(K) for j in range(N)])
outp = (C.c_void_p * K)(*[s[1] for s in singles])
secp = (C.c_void_p * K)(*[s[2] for s in singles])
nsec = (C.c_size_t * K)(*([WO] * K))
hffp = hff.ctypes.data_as(i64p)


def ok(st):
    if st != 0:
        raise RuntimeError(L.amph_last_error().decode())


def host_singles_rv():
    for arr, o, _, f in singles:
        ok(L.amph_recombine_verify(ctx._h, arr, N, o, f, 0, None))


def host_singles_mask():
    for arr, o, s, f in singles:
        ok(L.amph_mask_input(ctx._h, arr, N, s, WO, o, f, 0, None))


# device mode: K enqueued device calls against one packed call, one synchronise each
dout = torch.empty((T, 16), dtype=torch.uint8, device="cuda")
dff = torch.empty(K, dtype=torch.int64, device="cuda")
dsingles = []
for o in range(K):
    arr = (_lib._AmphOdo * N)(*[odo_struct(bbuf, j, o * WO, WO, dev_ptr) for j in range(N)])
    dsingles.append((arr, dout.data_ptr() + 16 * o * WO, bsec.data_ptr() + 16 * o * WO,
                     C.cast(C.c_void_p(dff.data_ptr() + 8 * o), i64p)))
dpacked = (_lib._AmphOdo * N)(*[odo_struct(bbuf, j, 0, T, dev_ptr) for j in range(N)])


def dev_singles_rv():
    for arr, o, _, f in dsingles:
        ok(L.amph_recombine_verify(ctx._h, arr, N, o, f, F_DEV, stream))
    torch.cuda.synchronize()


def dev_singles_mask():
    for arr, o, s, f in dsingles:
        ok(L.amph_mask_input(ctx._h, arr, N, s, WO, o, f, F_DEV, stream))
    torch.cuda.synchronize()


def dev_packed_rv():
    ok(L.amph_recombine_verify_packed(ctx._h, dpacked, N, doff.data_ptr(), K, dout.data_ptr(), dff.data_ptr(),
                                      F_DEV, stream))
    torch.cuda.synchronize()


def dev_packed_mask():
    ok(L.amph_mask_input_packed(ctx._h, dpacked, N, doff.data_ptr(), K, bsec.data_ptr(), dout.data_ptr(),
                                dff.data_ptr(), F_DEV, stream))
    torch.cuda.synchronize()


breps = max(5, a.reps // 2)
bat = alternate({
    "host_256_recombine_verify": host_singles_rv,
    "host_recombine_verify_batch": lambda: ok(L.amph_recombine_verify_batch(ctx._h, gathered, N, K, outp, hffp, 0)),
    "host_256_mask_input": host_singles_mask,
    "host_mask_input_batch": lambda: ok(L.amph_mask_input_batch(ctx._h, gathered, N, K, secp, nsec, outp, hffp, 0)),
    "device_256_recombine_verify": dev_singles_rv,
    "device_recombine_verify_packed": dev_packed_rv,
    "device_256_mask_input": dev_singles_mask,
    "device_mask_input_packed": dev_packed_mask,
}, breps, 3, wall_ms)
bat["speedup"] = {
    "host_recombine_verify": ratio(bat, "host_256_recombine_verify", "host_recombine_verify_batch"),
    "host_mask_input": ratio(bat, "host_256_mask_input", "host_mask_input_batch"),
    "device_recombine_verify": ratio(bat, "device_256_recombine_verify", "device_recombine_verify_packed"),
    "device_mask_input": ratio(bat, "device_256_mask_input", "device_mask_input_packed"),
}
result["batching"] = {"objects": K, "words_per_object": WO, "timing": "wall clock, one synchronise per side",
                      "reps": breps, **bat}

line = json.dumps(result)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
