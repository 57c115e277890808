"""The client session for K secrets against the packed calls and against a
loop of single sessions, on the same texts.

    python tools/bench_clients_session.py [--words T] [--parties N] [--objects 1,64,1024]
                                          [--reps R] [--warmup W] [--out FILE]

T words in total are split into K equal objects (K in --objects); every party's
responses are five slotted field buffers (the dense layout of
include/amphora_wire_batch.h), coded on the device by amph_odo_fields_b64_packed
from synthetic honest ODOs (amph_synth_odos, seeded); no reference data is read.

Three forms, for the verify finish and for the mask-to-JSON finish:

  packed   amph_recombine_verify_b64_packed / amph_mask_input_json_packed on all
           parties' buffers at once (one launch)
  loop     K single amph_client_* sessions one after the other, each with its
           begin, N party calls, finish and free (what a client had before)
  session  amph_clients_*: begin, N party calls (party_ms[j], arrival order),
           finish; tail_ms = the last party call + the finish, total_ms = all

Host mode: the buffers are pageable host memory, the host clock runs around
calls that end in a device synchronisation.  Device mode: the buffers are
resident, HIP events on one stream bracket each form (device time of the
sequence, launch gaps included).  The forms alternate inside each repetition;
medians over --reps repetitions after --warmup, with min and max.  The outputs
of the three forms are compared byte for byte before anything is timed.
Launch counts come from amph_ctx_stats, copies from amph_clients_copies.
Prints one JSON line; --out also writes it to a file.
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
import amphora_amd as A  # noqa: E402
from amphora_amd.spdz import TEST_PRIME, TEST_R, TEST_RINV  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--words", type=int, default=1 << 22)
ap.add_argument("--parties", type=int, default=3)
ap.add_argument("--objects", default="1,64,1024")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--modes", default="host,device")
ap.add_argument("--out", default=None)
a = ap.parse_args()
T, n = a.words, a.parties
if not torch.cuda.is_available():
    sys.exit("bench_clients_session: no GPU (there is no CPU fallback)")
ctx = A.Context(TEST_PRIME, TEST_R, TEST_RINV)
LIB = A._lib
L = LIB.lib
F_DEVICE = 1


def ok(st):
    if st != 0:
        raise RuntimeError("status %d: %s" % (st, L.amph_last_error().decode()))


def med(xs):
    return round(statistics.median(xs), 4)


def spread(xs):
    return {"median_ms": med(xs), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4)}


def launches():
    return ctx.stats()["kernel_launches"]


_, slab, _ = ctx.synth_odos(seed=1, n=n, words=T, noncanon_permille=20)
secrets_d = ctx.synth_words(2, T)
torch.cuda.synchronize()


class Setup:
    """K equal objects of T // K words: tables, every party's slotted buffers
    on the device and (lazily) in pageable host memory, per-object structs."""

    def __init__(self, K):
        self.K = K
        W = T // K
        self.sizes = [W] * (K - 1) + [T - W * (K - 1)]
        self.woff = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.uint64)
        self.nc = [LIB.wire_text_chars(w) for w in self.sizes]
        self.foff = np.concatenate([[0], np.cumsum([(c + 15) & ~15 for c in self.nc])]).astype(np.uint64)
        self.field_chars, self.foff = int(self.foff[-1]), self.foff[:-1]
        ul = [37 * w + 1 if w else 2 for w in self.sizes]
        self.uoff = np.concatenate([[0], np.cumsum([(u + 15) & ~15 for u in ul])]).astype(np.uint64)
        self.upload_chars, self.uoff, self.ulen = int(self.uoff[-1]), self.uoff[:-1], ul
        self.dev = []
        for j in range(n):
            out, _ = ctx.odo_fields_b64_packed([slab[k, j] for k in range(5)], self.woff)  # the dense layout
            self.dev.append([b[:self.field_chars] for b in out])
        torch.cuda.synchronize()
        self.woff_d = torch.from_numpy(self.woff.astype(np.int64)).cuda()
        self.foff_d = torch.from_numpy(self.foff.astype(np.int64)).cuda()
        self.uoff_d = torch.from_numpy(self.uoff.astype(np.int64)).cuda()

    def bufs(self, dev):
        if dev:
            return self.dev
        if not hasattr(self, "host"):
            self.host = [[b.cpu().numpy().copy() for b in five] for five in self.dev]
        return self.host


def base_ptr(x):
    return x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data


def run_mode(S, dev, mask):
    """One K, one memory mode, one finish: the three forms, alternating."""
    K = S.K
    bufs = S.bufs(dev)
    all_arr, _k1 = ctx._text_structs(bufs)
    one_arr = [ctx._text_structs([bufs[j]])[0] for j in range(n)]
    # the single sessions' texts: object o's slice of every buffer (pointer + its own length)
    single = [[LIB._AmphOdoB64(*[base_ptr(bufs[j][k]) + int(S.foff[o]) for k in range(5)], S.nc[o])
               for j in range(n)] for o in range(K)]
    if dev:
        sec = secrets_d
        mk = lambda shape, dt=torch.uint8: torch.zeros(shape, dtype=dt, device="cuda")  # noqa: E731
        wo, fo, uo = S.woff_d, S.foff_d, S.uoff_d
        stream = torch.cuda.Stream()
        sp = C.c_void_p(stream.cuda_stream)
    else:
        sec = np.ascontiguousarray(secrets_d.cpu().numpy())
        mk = lambda shape, dt=np.uint8: np.zeros(shape, dt)  # noqa: E731
        wo, fo, uo = S.woff, S.foff, S.uoff
        stream, sp = None, None
    P = base_ptr
    nout = S.upload_chars if mask else 16 * T
    outs = [mk(nout) for _ in range(3)]  # packed, loop, session
    ffs = [mk(K, torch.int64 if dev else np.int64) for _ in range(3)]
    bads = [mk(K, torch.int64 if dev else np.int64) for _ in range(3 + n)]
    flags = F_DEVICE if dev else 0
    if dev:  # the zero fills ran on torch's current stream: done before the session's stream writes the arrays
        torch.cuda.synchronize()

    def packed():
        if mask:
            ok(L.amph_mask_input_json_packed(ctx._h, all_arr, n, P(wo), P(fo), K, P(sec), P(outs[0]), nout, P(uo),
                                             P(ffs[0]), P(bads[0]), flags, sp))
        else:
            ok(L.amph_recombine_verify_b64_packed(ctx._h, all_arr, n, P(wo), P(fo), K, P(outs[0]), P(ffs[0]),
                                                  P(bads[0]), flags, sp))

    def loop():
        for o in range(K):
            W, a0 = S.sizes[o], int(S.woff[o])
            h = C.c_void_p()
            ok(L.amph_client_begin_dev(ctx._h, W, n, sp, C.byref(h)) if dev else
               L.amph_client_begin(ctx._h, W, n, C.byref(h)))
            ffp = C.cast(C.c_void_p(P(ffs[1]) + 8 * o), C.POINTER(C.c_int64))
            bdp = C.cast(C.c_void_p(P(bads[1]) + 8 * o), C.POINTER(C.c_int64))
            for j in range(n):
                ok(L.amph_client_party_dev(h, j, C.byref(single[o][j]), bdp, sp) if dev else
                   L.amph_client_party(h, j, C.byref(single[o][j]), bdp))
            if mask:
                dst, cap = P(outs[1]) + int(S.uoff[o]), S.ulen[o]
                ok(L.amph_client_finish_mask_json_dev(h, P(sec) + 16 * a0, W, dst, cap, ffp, bdp, sp) if dev else
                   L.amph_client_finish_mask_json(h, P(sec) + 16 * a0, W, dst, cap, ffp, bdp))
            else:
                dst = P(outs[1]) + 16 * a0
                ok(L.amph_client_finish_verify_dev(h, dst, ffp, bdp, sp) if dev else
                   L.amph_client_finish_verify(h, dst, ffp, bdp))
            L.amph_client_free(h)

    def session(marks):
        """marks(i): a time stamp after step i (begin, each party, finish)."""
        h = C.c_void_p()
        ok(L.amph_clients_begin_dev(ctx._h, S.woff.ctypes.data, K, n, sp, C.byref(h)) if dev else
           L.amph_clients_begin(ctx._h, S.woff.ctypes.data, K, n, C.byref(h)))
        marks(0)
        for j in range(n):
            ok(L.amph_clients_party_dev(h, j, one_arr[j], P(bads[3 + j]), sp) if dev else
               L.amph_clients_party(h, j, one_arr[j], P(bads[3 + j])))
            marks(1 + j)
        if mask:
            ok(L.amph_clients_finish_mask_json_dev(h, P(sec), P(outs[2]), nout, P(ffs[2]), P(bads[2]), sp) if dev else
               L.amph_clients_finish_mask_json(h, P(sec), P(outs[2]), nout, P(ffs[2]), P(bads[2])))
        else:
            ok(L.amph_clients_finish_verify_dev(h, P(outs[2]), P(ffs[2]), P(bads[2]), sp) if dev else
               L.amph_clients_finish_verify(h, P(outs[2]), P(ffs[2]), P(bads[2])))
        marks(n + 1)
        return h

    rows = {"packed": [], "loop": [], "begin": [], "party": [[] for _ in range(n)], "finish": []}
    counts = {}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 7)] if dev else None
    for rep in range(a.warmup + a.reps):
        if dev:
            with torch.cuda.stream(stream):
                l0 = launches()
                ev[0].record(stream)
                packed()
                ev[1].record(stream)
                l1 = launches()
                ev[2].record(stream)
                loop()
                ev[3].record(stream)
                l2 = launches()
                ev[4].record(stream)
                h = session(lambda i: ev[5 + i].record(stream))
                l3 = launches()
                L.amph_clients_free(h)  # waits for the stream
                stream.synchronize()
            t = [ev[0].elapsed_time(ev[1]), ev[2].elapsed_time(ev[3])] + \
                [ev[4 + i].elapsed_time(ev[5 + i]) for i in range(n + 2)]
        else:
            st = []
            l0 = launches()
            t0 = time.perf_counter()
            packed()
            t1 = time.perf_counter()
            l1 = launches()
            loop()
            t2 = time.perf_counter()
            l2 = launches()
            c0 = ctx.clients_copies()
            h = session(lambda i: st.append(time.perf_counter()))
            l3 = launches()
            counts["session_copies"] = ctx.clients_copies() - c0
            L.amph_clients_free(h)
            st = [t2] + st
            t = [1e3 * (t1 - t0), 1e3 * (t2 - t1)] + [1e3 * (y - x) for x, y in zip(st, st[1:])]
        counts.update(packed_launches=l1 - l0, loop_launches=l2 - l1, session_launches=l3 - l2)
        if rep == 0:  # clean verdicts, then the three forms agree, before anything is timed
            host = lambda x: x.cpu().numpy() if dev else x  # noqa: E731
            clean = -1 if not dev else 0x7F7F7F7F7F7F7F7F
            names = ["packed ff", "loop ff", "session ff", "packed bad", "loop bad", "session bad"] + \
                ["party %d bad" % j for j in range(n)]
            for name, v in zip(names, ffs + bads):
                set_ = np.nonzero(host(v) != clean)[0]
                if set_.size:
                    raise RuntimeError("K=%d %s: %d verdicts set, first object %d = %d" % (
                        K, name, set_.size, set_[0], host(v)[set_[0]]))
            o0, o1, o2 = (host(x) for x in outs)
            for o in range(K):
                lo = int(S.uoff[o]) if mask else 16 * int(S.woff[o])
                hi = lo + (S.ulen[o] if mask else 16 * S.sizes[o])
                for name, x in (("loop", o1), ("session", o2)):
                    if not np.array_equal(o0[lo:hi], x[lo:hi]):
                        at = int(np.nonzero(o0[lo:hi] != x[lo:hi])[0][0])
                        raise RuntimeError("K=%d object %d: the %s's output differs from the packed call's at byte %d "
                                           "of %d" % (K, o, name, at, hi - lo))
        if rep < a.warmup:
            continue
        rows["packed"].append(t[0])
        rows["loop"].append(t[1])
        rows["begin"].append(t[2])
        for j in range(n):
            rows["party"][j].append(t[3 + j])
        rows["finish"].append(t[3 + n])
    tails = [rows["party"][n - 1][i] + rows["finish"][i] for i in range(a.reps)]
    totals = [rows["begin"][i] + sum(rows["party"][j][i] for j in range(n)) + rows["finish"][i] for i in range(a.reps)]
    res = {"packed": spread(rows["packed"]), "loop_of_single_sessions": spread(rows["loop"]),
           "session": {"begin_ms": med(rows["begin"]), "party_ms": [med(x) for x in rows["party"]],
                       "finish_ms": med(rows["finish"]), "tail": spread(tails), "total": spread(totals)}}
    res.update(counts)
    res["tail_over_packed"] = round(res["session"]["tail"]["median_ms"] / res["packed"]["median_ms"], 4)
    res["total_over_loop"] = round(res["session"]["total"]["median_ms"] / res["loop_of_single_sessions"]["median_ms"], 4)
    return res


res = {"tool": "bench_clients_session", "device": torch.cuda.get_device_name(0), "words_total": T, "parties": n,
       "reps": a.reps, "warmup": a.warmup, "host_memory": "pageable",
       "timing": {"host": "host clock around calls that end in a device synchronisation",
                  "device": "device time between HIP events on one stream, launch gaps included"},
       "bytes_per_word": {"session_per_party": round(5 * (64 / 3 + 16 + 16), 1), "session_finish": 96,
                          "packed_per_party": round(5 * 64 / 3, 1), "packed_output": 16},
       "objects": {}}
for K in [int(x) for x in a.objects.split(",")]:
    S = Setup(K)
    row = {"words_per_object": S.sizes[0], "field_chars": S.field_chars}
    for mode in a.modes.split(","):
        row[mode] = {"verify": run_mode(S, mode == "device", False), "mask_json": run_mode(S, mode == "device", True)}
    res["objects"][str(K)] = row
    del S
line = json.dumps(res)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
