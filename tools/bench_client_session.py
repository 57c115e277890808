"""The client session against the whole calls, on the same texts.

    python tools/bench_client_session.py [--words W] [--parties N] [--reps R] [--out FILE]

Host mode (the default question): a client holds each party's five base64
field texts in pageable host memory, as an HTTP client does.

  whole_ms          amph_recombine_verify_b64 on all 5 N texts (the baseline:
                    upload of every text, one launch, secrets back)
  party_ms[j]       amph_client_party for party j (upload of ITS five texts,
                    one launch, one synchronisation), in arrival order
  finish_ms         amph_client_finish_verify (one launch, secrets back)
  tail_ms           party_ms[last] + finish_ms: the work left once the last
                    response is in, the rest having hidden behind the arrivals
  session_total_ms  begin + every party + finish

and the same with the mask-to-JSON finish against amph_mask_input_json.  Every
figure is the median over --reps repetitions (after --warmup), host clock
around calls that end in a device synchronisation; whole call and session
alternate inside each repetition, outputs go to buffers allocated once.  The
outputs of both forms are compared byte for byte before anything is timed.

One device-mode line: all texts already on the device, HIP events around the
whole call's launch and around the session's begin + N party launches + finish
on one stream (device time of the sequence, launch gaps included).

Inputs are synthetic honest ODOs (amph_synth_odos, seeded), base64-coded on
the host; no reference data is read.  Prints one JSON line; --out also writes
it to a file.
"""
import argparse
import base64
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import amphora_amd as A  # noqa: E402
from amphora_amd.spdz import TEST_PRIME, TEST_R, TEST_RINV  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--words", type=int, default=1 << 22)
ap.add_argument("--parties", type=int, default=3)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=None)
a = ap.parse_args()
W, n = a.words, a.parties
if not torch.cuda.is_available():
    sys.exit("bench_client_session: no GPU (there is no CPU fallback)")
ctx = A.Context(TEST_PRIME, TEST_R, TEST_RINV)
L = A._lib.lib
i64p = C.POINTER(C.c_int64)

# ---- inputs: honest ODOs generated on the device, coded as text on the host ----------
_, slab, _ = ctx.synth_odos(seed=1, n=n, words=W, noncanon_permille=20)
torch.cuda.synchronize()
host = slab.cpu().numpy()
texts = [[np.frombuffer(base64.b64encode(host[k, j].tobytes()), np.uint8) for k in range(5)] for j in range(n)]
del host
nchars = texts[0][0].size
secrets = np.ascontiguousarray(ctx.synth_words(2, W).cpu().numpy())
all_arr, _keep_all = ctx._text_structs(texts)
one_arr = [ctx._text_structs([texts[j]])[0] for j in range(n)]
out_y = [np.zeros((W, 16), np.uint8) for _ in range(2)]
cap = 37 * W + 1
out_t = [np.zeros(cap, np.uint8) for _ in range(2)]
ff, bad = C.c_int64(), C.c_int64()


def ok(st):
    if st != 0:
        raise RuntimeError("status %d: %s" % (st, L.amph_last_error().decode()))


def whole(mask):
    t0 = time.perf_counter()
    if mask:
        ok(L.amph_mask_input_json(ctx._h, all_arr, n, W, secrets.ctypes.data, W, out_t[0].ctypes.data, cap,
                                  C.byref(ff), C.byref(bad), 0, None))
    else:
        ok(L.amph_recombine_verify_b64(ctx._h, all_arr, n, W, out_y[0].ctypes.data, C.byref(ff), C.byref(bad), 0,
                                       None))
    return 1e3 * (time.perf_counter() - t0)


def session(mask):
    """-> (begin_ms, [party_ms], finish_ms)"""
    h = C.c_void_p()
    t = [time.perf_counter()]
    ok(L.amph_client_begin(ctx._h, W, n, C.byref(h)))
    t.append(time.perf_counter())
    for j in range(n):
        ok(L.amph_client_party(h, j, one_arr[j], C.byref(bad)))
        t.append(time.perf_counter())
    if mask:
        ok(L.amph_client_finish_mask_json(h, secrets.ctypes.data, W, out_t[1].ctypes.data, cap, C.byref(ff),
                                          C.byref(bad)))
    else:
        ok(L.amph_client_finish_verify(h, out_y[1].ctypes.data, C.byref(ff), C.byref(bad)))
    t.append(time.perf_counter())
    L.amph_client_free(h)
    d = [1e3 * (y - x) for x, y in zip(t, t[1:])]
    return d[0], d[1:1 + n], d[-1]


def med(xs):
    return round(statistics.median(xs), 4)


def host_rows(mask):
    rows = {"whole": [], "begin": [], "party": [[] for _ in range(n)], "finish": []}
    for rep in range(a.warmup + a.reps):
        w = whole(mask)
        b, p, f = session(mask)
        if rep == 0:  # the two forms agree before anything is timed
            same = np.array_equal(out_t[0], out_t[1]) if mask else np.array_equal(out_y[0], out_y[1])
            if not same or ff.value != -1:
                raise RuntimeError("the session's output differs from the whole call's")
        if rep < a.warmup:
            continue
        rows["whole"].append(w)
        rows["begin"].append(b)
        rows["finish"].append(f)
        for j in range(n):
            rows["party"][j].append(p[j])
    party = [med(x) for x in rows["party"]]
    totals = [rows["begin"][i] + sum(rows["party"][j][i] for j in range(n)) + rows["finish"][i]
              for i in range(a.reps)]
    tails = [rows["party"][n - 1][i] + rows["finish"][i] for i in range(a.reps)]
    return {"whole_ms": med(rows["whole"]), "whole_ms_min_max": [round(min(rows["whole"]), 4),
                                                                 round(max(rows["whole"]), 4)],
            "begin_ms": med(rows["begin"]), "party_ms": party, "finish_ms": med(rows["finish"]),
            "tail_ms": med(tails), "tail_ms_min_max": [round(min(tails), 4), round(max(tails), 4)],
            "session_total_ms": med(totals)}


# ---- device mode: texts resident, device time of each form's launches -------------------
def device_row():
    dt = [[torch.from_numpy(t.copy()).cuda() for t in p] for p in texts]
    darr, _k = ctx._text_structs(dt)
    done = [ctx._text_structs([p])[0] for p in dt]
    dy = [torch.empty((W, 16), dtype=torch.uint8, device="cuda") for _ in range(2)]
    v = torch.empty(4 + n, dtype=torch.int64, device="cuda")
    vp = [C.cast(C.c_void_p(v[i:].data_ptr()), i64p) for i in range(4 + n)]
    s = torch.cuda.Stream()
    sp = C.c_void_p(s.cuda_stream)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    tw, ts = [], []
    with torch.cuda.stream(s):
        for rep in range(a.warmup + a.reps):
            ev[0].record(s)
            ok(L.amph_recombine_verify_b64(ctx._h, darr, n, W, dy[0].data_ptr(), vp[0], vp[1], 1, sp))
            ev[1].record(s)
            h = C.c_void_p()
            ev[2].record(s)
            ok(L.amph_client_begin_dev(ctx._h, W, n, sp, C.byref(h)))
            for j in range(n):
                ok(L.amph_client_party_dev(h, j, done[j], vp[4 + j], sp))
            ok(L.amph_client_finish_verify_dev(h, dy[1].data_ptr(), vp[2], vp[3], sp))
            ev[3].record(s)
            L.amph_client_free(h)  # waits for the stream
            s.synchronize()
            if rep == 0 and not torch.equal(dy[0], dy[1]):
                raise RuntimeError("device mode: the session's secrets differ from the whole call's")
            if rep >= a.warmup:
                tw.append(ev[0].elapsed_time(ev[1]))
                ts.append(ev[2].elapsed_time(ev[3]))
    return {"whole_ms": med(tw), "session_ms": med(ts), "what": "device time between events on one stream"}


res = {"tool": "bench_client_session", "device": torch.cuda.get_device_name(0), "words": W, "parties": n,
       "reps": a.reps, "warmup": a.warmup, "nchars_per_field": int(nchars),
       "text_bytes_per_party": int(5 * nchars), "host_memory": "pageable",
       "verify": host_rows(False), "mask_json": host_rows(True), "device_mode_verify": device_row()}
for k in ("verify", "mask_json"):
    res[k]["tail_over_whole"] = round(res[k]["tail_ms"] / res[k]["whole_ms"], 4)
    res[k]["total_over_whole"] = round(res[k]["session_total_ms"] / res[k]["whole_ms"], 4)
line = json.dumps(res)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
