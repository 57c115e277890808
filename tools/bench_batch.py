"""Many secrets in one call: what the segmented kernels cost on the hot path
and what batching buys ("Packed calls").

    python tools/bench_batch.py [--reps R] [--out FILE]

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
