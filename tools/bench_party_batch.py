"""A/B of the party side's device-resident session over many requests
(DESIGN.md 4c-next): party 0 of three answers K requests of W words each,
the partners' texts already on the device.

  A  K single amph_party_*_dev sessions in sequence on one stream, each begun,
     given its two partner texts, finished and freed (amph_party_free waits
     for the stream, as a server does before it reuses the buffers);
  B  one amph_parties_*_dev session over the K requests, freed likewise.

Device events go around the whole request set and the window ends in a
synchronise.  Every shape is warmed, A and B alternate in one process, the
medians and the spread of at least 20 repetitions are reported, and both
outputs go through the same oracle check at the timed sizes (a seeded sample
of objects, every word of each).  Refuses to run without a GPU.

    python tools/bench_party_batch.py [--reps 20] [--shapes 1024x4096,64x65536,1x4194304] [--out profiles/party_batch.json]
"""
from __future__ import annotations

import argparse
import base64
import json
import os
import random
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default="1024x4096,64x65536,1x4194304")
    ap.add_argument("--sample", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "party_batch.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_party_batch: no GPU -- nothing is measured without one")
    import amphora_amd as A
    from oracle import amphora_oracle as O
    from oracle import coracle
    assert args.reps >= 20, "at least 20 repetitions"
    ctx = A.Context(O.TEST_PRIME, O.TEST_R, O.TEST_RINV)
    F = coracle.test_field(threads=16)
    n, results = 3, []
    for shape in args.shapes.split(","):
        K, W = (int(x) for x in shape.split("x"))
        T = K * W
        woff = np.arange(K + 1, dtype=np.uint64) * W
        inp = [(ctx.synth_words(11 + j, 2 * T).view(T, 32), ctx.synth_words(21 + j, 4 * T).view(2 * T, 32),
                ctx.synth_words(31 + j, 12 * T).view(2 * T, 96)) for j in range(n)]
        partners = [ctx.parties_begin_dev(inp[j][0], 32, inp[j][1], inp[j][2], woff, n) for j in (1, 2)]
        ptext = [p.text_dev() for p in partners]
        torch.cuda.synchronize()
        toff = [int(x) for x in partners[0].text_offsets]
        plens = [[int(x) for x in t[2].cpu().numpy()] for t in ptext]
        sh, mk, tr = inp[0]

        def run_a(keep=()):
            got = {}
            for o in range(K):
                a, b = o * W, (o + 1) * W
                s = ctx.party_begin_dev(sh[a:b], 32, mk[2 * a:2 * b], tr[2 * a:2 * b], n)
                for slot in (1, 2):
                    t, ln = ptext[slot - 1][0], plens[slot - 1][o]
                    s.partner(slot, t[toff[o]:toff[o] + ln])
                f = s.finish_b64(True)
                if o in keep:
                    got[o] = [x.cpu().numpy().tobytes() for x in f]
                s.close()
            return got

        def run_b(keep=()):
            s = ctx.parties_begin_dev(sh, 32, mk, tr, woff, n)
            for slot in (1, 2):
                s.partner(slot, ptext[slot - 1][0], ptext[slot - 1][2])
            f = s.finish_b64(True)
            got = {}
            if keep:
                per = s.split_fields([x.cpu().numpy() for x in f])
                got = {o: per[o] for o in keep}
            s.close()
            return got

        # the oracle check of both at this size
        sample = sorted(random.Random(K * 1000003 + W).sample(range(K), min(args.sample, K)))
        ga, gb = run_a(sample), run_b(sample)
        for o in sample:
            a, b = o * W, (o + 1) * W
            host = [[x[lo:hi].cpu().numpy() for x, (lo, hi) in zip(inp[j], ((a, b), (2 * a, 2 * b), (2 * a, 2 * b)))]
                    for j in range(n)]
            pre = [F.odo_pre(h[0], 32, h[1], h[2]) for h in host]
            opened = F.recombine_diffs([p[3] for p in pre], [p[4] for p in pre])
            ow, ou = F.odo_post(opened, host[0][2], True)
            want = [base64.b64encode(x.tobytes()) for x in (pre[0][0], pre[0][1], pre[0][2], ow, ou)]
            assert ga[o] == want, "A differs from the oracle at object %d of %s" % (o, shape)
            assert gb[o] == want, "B differs from the oracle at object %d of %s" % (o, shape)
        for fn in (run_a, run_b, run_a, run_b):  # warm: code objects, the pool
            fn()
        torch.cuda.synchronize()
        times = {"A": [], "B": []}
        for _ in range(args.reps):
            for name, fn in (("A", run_a), ("B", run_b)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1))
        row = {"objects": K, "words_each": W, "parties": n, "reps": args.reps, "oracle_checked_objects": sample}
        for name, v in times.items():
            v = sorted(v)
            row[name] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(v[0], 4),
                         "max_ms": round(v[-1], 4), "p10_ms": round(v[len(v) // 10], 4),
                         "p90_ms": round(v[(9 * len(v)) // 10], 4)}
        row["B_over_A"] = round(row["B"]["median_ms"] / row["A"]["median_ms"], 4)
        results.append(row)
        print("%5d x %8d words: A %.3f ms (%.3f-%.3f)  B %.3f ms (%.3f-%.3f)  B/A %.3f" % (
            K, W, row["A"]["median_ms"], row["A"]["min_ms"], row["A"]["max_ms"], row["B"]["median_ms"],
            row["B"]["min_ms"], row["B"]["max_ms"], row["B_over_A"]), flush=True)
        for p in partners:
            p.close()
        del inp, partners, ptext
        torch.cuda.empty_cache()
    line = json.dumps({"bench": "party_batch", "device": torch.cuda.get_device_name(0), "build": A._lib.build_id(),
                       "what": "party 0 of 3, device mode, begin + 2 partners + finish_b64 + free per request set",
                       "shapes": results})
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
