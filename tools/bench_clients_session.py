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

--bodies (include/amphora_client_bodies.h): instead of the above, every party's
K responses as K JSON bodies with the five members inside, and three pairs of
forms on the same texts, alternating inside each repetition:

  device   the N accumulate launches of a device-mode session: amph_clients_party_dev
           on the slotted buffers against amph_bodies_party_dev on ONE device buffer
           that holds the bodies (its starts upload included); HIP events.  Run
           under rocprofv3 --kernel-trace --stats this gives the two kernel forms.
  host     amph_clients_party on the (already gathered) slotted buffers against
           amph_bodies_party on the K bodies, per party call; host clock
  python   ResponseSessions.add_bodies for all parties, in_place=True against
           in_place=False (the scan in C and no gather, against
           wire.odo_field_texts and the per-object, per-field gather); host clock

The secrets of the two forms of each pair are compared before anything is timed.
--variant-lib LIB adds the device pair a third form, "bodies_variant": the same
calls through a second library built from the same tree with another fetch
(-DAMPH_BODY_FETCH=1: one unaligned 16-byte load per lane and field instead of
two aligned ones and the funnel).
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
ap.add_argument("--bodies", action="store_true", help="the body calls against the slotted calls")
ap.add_argument("--variant-lib", default=None,
                help="--bodies, device mode: a library built with -DAMPH_BODY_FETCH=1 (tools/build_native.py "
                     "build_variant): its amph_bodies_party_dev as a third form, in the same process")
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


def bodies_of(S):
    """Per party the K response bodies (bytes) cut from the host slotted
    buffers, and their (K, 5) member starts (amph_bodies_scan)."""
    host = S.bufs(False)
    head = b'{"secretId":"00000000-0000-0000-0000-00000000002a","tags":[{"key":"k","value":"v","valueType":"STRING"}]'
    bodies, starts = [], []
    for j in range(n):
        bs, st = [], np.empty((S.K, 5), np.uint64)
        for o in range(S.K):
            a0, nc = int(S.foff[o]), S.nc[o]
            bs.append(head + b"".join(b',"%s":"' % name.encode() + host[j][k][a0:a0 + nc].tobytes() + b'"'
                                      for k, name in enumerate(LIB.ODO_FIELD_NAMES)) + b"}")
            st[o], lens = LIB.bodies_scan(bs[-1])
            assert (lens == nc).all()
        bodies.append(bs)
        starts.append(st)
    return bodies, starts


def run_bodies(S):
    from amphora_amd import client
    K = S.K
    bodies, starts = bodies_of(S)
    host = S.bufs(False)
    out = {"body_bytes_per_party": sum(len(b) for b in bodies[0]), "slotted_bytes_per_party": 5 * S.field_chars}

    def finish(s):
        y = s.finish_verify()[0]
        if s.dev:
            torch.cuda.synchronize()
        return y.cpu().numpy() if s.dev else y

    V = vctx = None
    if a.variant_lib and "device" in a.modes.split(","):
        V = C.CDLL(os.path.abspath(a.variant_lib))
        vp = C.c_void_p
        V.amph_ctx_create.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(vp)]
        V.amph_clients_begin_dev.argtypes = [vp, vp, C.c_size_t, C.c_int, vp, C.POINTER(vp)]
        V.amph_bodies_party_dev.argtypes = [vp, C.c_int, vp, C.c_size_t, vp, vp]
        V.amph_clients_finish_verify_dev.argtypes = [vp, vp, vp, vp, vp]
        V.amph_clients_free.argtypes = [vp]
        V.amph_clients_free.restype = None
        V.amph_last_error.restype = C.c_char_p
        vctx = vp()
        keys = [LIB.le16(x) for x in (TEST_PRIME, TEST_R, TEST_RINV)]
        if V.amph_ctx_create(*keys, 0, C.byref(vctx)) != 0:
            raise RuntimeError("variant context: %s" % V.amph_last_error().decode())

    def variant(check=False):
        """The N amph_bodies_party_dev calls through the variant library."""
        def vok(st):
            if st != 0:
                raise RuntimeError("variant status %d: %s" % (st, V.amph_last_error().decode()))
        h, sp = C.c_void_p(), C.c_void_p(stream.cuda_stream)
        vok(V.amph_clients_begin_dev(vctx, S.woff.ctypes.data, K, n, sp, C.byref(h)))
        ev[0].record(stream)
        for j in range(n):
            vok(V.amph_bodies_party_dev(h, j, dbufs[j].data_ptr(), dbufs[j].numel(), absolute[j].ctypes.data, sp))
        ev[1].record(stream)
        y = None
        if check:
            y = torch.zeros((T, 16), dtype=torch.uint8, device="cuda")
            ff, bad = (torch.zeros(K, dtype=torch.int64, device="cuda") for _ in range(2))
            torch.cuda.synchronize()
            vok(V.amph_clients_finish_verify_dev(h, y.data_ptr(), ff.data_ptr(), bad.data_ptr(), sp))
        V.amph_clients_free(h)  # waits for the stream
        stream.synchronize()
        return [ev[0].elapsed_time(ev[1])], (y.cpu().numpy() if check else None)

    for mode in a.modes.split(","):
        dev = mode == "device"
        if dev:
            stream = torch.cuda.Stream()
            at = np.concatenate([[0], np.cumsum([(len(b) + 15) & ~15 for b in bodies[0]])]).astype(np.uint64)
            dbufs, absolute = [], []
            for j in range(n):
                buf = np.zeros(int(at[-1]) + 16, np.uint8)
                for b, x in zip(bodies[j], at):
                    buf[int(x):int(x) + len(b)] = np.frombuffer(b, np.uint8)
                dbufs.append(torch.from_numpy(buf).cuda())
                absolute.append(starts[j] + at[:-1, None])
            torch.cuda.synchronize()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

        def one(form, check=False):
            """-> ms of the N party calls (device: events around them; host: per call, summed)."""
            s = ctx.clients_begin_dev(S.woff, n, stream) if dev else ctx.clients_begin(S.woff, n)
            per = []
            with s:
                if dev:
                    ev[0].record(stream)
                for j in range(n):
                    t0 = time.perf_counter()
                    if form == "slotted":
                        s.party(j, S.dev[j] if dev else host[j])
                    elif dev:
                        s.party_bodies_dev(j, dbufs[j], absolute[j])
                    else:
                        s.party_bodies(j, bodies[j], starts[j])
                    per.append(1e3 * (time.perf_counter() - t0))
                if dev:
                    ev[1].record(stream)
                    stream.synchronize()
                    per = [ev[0].elapsed_time(ev[1])]
                y = finish(s) if check else None
                if dev:
                    torch.cuda.synchronize()
            return per, y

        (_, y0), (_, y1) = one("slotted", True), one("bodies", True)
        if not np.array_equal(y0, y1):
            raise RuntimeError("K=%d %s: the body form's secrets differ from the slotted form's" % (K, mode))
        rows = {"slotted": [], "bodies": []}
        if dev and V is not None:
            rows["bodies_variant"] = []
            if not np.array_equal(y0, variant(True)[1]):
                raise RuntimeError("K=%d: the variant library's secrets differ from the slotted form's" % K)
        for rep in range(a.warmup + a.reps):
            for form in rows:
                per, _ = variant() if form == "bodies_variant" else one(form)
                if rep >= a.warmup:
                    rows[form].append(per)
        res = {form: {"parties_total": spread([sum(p) for p in rows[form]]),
                      "party_ms": [med([p[j] for p in rows[form]]) for j in range(len(rows[form][0]))]}
               for form in rows}
        res["bodies_over_slotted"] = round(res["bodies"]["parties_total"]["median_ms"] /
                                           res["slotted"]["parties_total"]["median_ms"], 4)
        if "bodies_variant" in res:
            res["variant_over_bodies"] = round(res["bodies_variant"]["parties_total"]["median_ms"] /
                                               res["bodies"]["parties_total"]["median_ms"], 4)
        out[mode] = res
    if "host" in a.modes.split(","):
        util = client.SecretShareUtil(ctx)
        texts = [[b.decode("ascii") for b in bs] for bs in bodies]
        rows = {True: [], False: []}
        for rep in range(a.warmup + a.reps):
            for in_place in (True, False):
                with client.ResponseSessions(util, n, in_place=in_place) as rs:
                    t0 = time.perf_counter()
                    for j in range(n):
                        rs.add_bodies(j, texts[j])
                    t1 = time.perf_counter()
                    if rep == 0:  # the same secrets either way
                        got = rs.secrets()
                        if any(isinstance(g, Exception) for g in got):
                            raise RuntimeError("K=%d add_bodies(in_place=%s): %r" % (K, in_place, got[0]))
                        rows.setdefault("y", []).append([g[2] for g in got] if K <= 64 else None)
                if rep >= a.warmup:
                    rows[in_place].append(1e3 * (t1 - t0))
        if rows["y"][0] != rows["y"][1]:
            raise RuntimeError("K=%d: add_bodies in place and gathered give different secrets" % K)
        out["python_add_bodies"] = {"in_place": spread(rows[True]), "gather": spread(rows[False]),
                                    "in_place_over_gather": round(med(rows[True]) / med(rows[False]), 4)}
    return out


if a.bodies:
    res = {"tool": "bench_clients_session --bodies", "device": torch.cuda.get_device_name(0), "words_total": T,
           "parties": n, "reps": a.reps, "warmup": a.warmup, "host_memory": "pageable",
           "timing": {"host": "host clock around calls that end in a device synchronisation",
                      "device": "device time between HIP events around the N party calls on one stream"},
           "objects": {}}
    for K in [int(x) for x in a.objects.split(",")]:
        S = Setup(K)
        res["objects"][str(K)] = dict(run_bodies(S), words_per_object=S.sizes[0])
        del S
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    sys.exit(0)

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
