"""The upload hop on the MaskedInput JSON text against the launches it
replaces, device-resident, kernel time only.

    python tools/bench_upload_wire.py [--words W] [--parties N] [--reps R] [--out FILE]

Party side:  k_conv_json (amph_convert_share_json) against k_b64_unwords +
             k_conv (amph_base64_decode_words, then amph_convert_share).
Client side: k_mask_json (amph_mask_input_json) against k_mask_b64 writing the
             bare 24-character records (amph_mask_input_b64, out_records24).

Every kernel is timed by HIP events stamped by its own dispatch
(amph_time_next_launch); the candidates alternate inside one process, --reps
timed launches each after 3 warm-up rounds.  Prints (and with --out writes)
one JSON object: per kernel the median, quartiles, minimum and maximum in
microseconds, the fused-over-replaced ratios, and whether each fused kernel's
median is within the spread (max - min) observed for what it replaces.  The
outputs of both paths are compared once, byte for byte, before timing.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import amphora_amd as A  # noqa: E402
from amphora_amd.spdz import TEST_PRIME, TEST_R, TEST_RINV  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--words", type=int, default=1 << 22)
ap.add_argument("--parties", type=int, default=3)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--out", default=None)
a = ap.parse_args()
W, n = a.words, a.parties
NF = A._lib.AMPH_NO_FAILURE
ctx = A.Context(TEST_PRIME, TEST_R, TEST_RINV)
L = A._lib.lib
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
for e in ev:
    e.record()
torch.cuda.synchronize()


def kernel_us(fn):
    """fn's (single) kernel launch, timed by its own dispatch."""
    L.amph_time_next_launch(ev[0].cuda_event, ev[1].cuda_event)
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * ev[0].elapsed_time(ev[1]), out


def frame(records):
    """(W, 24) device records -> the "data" array text, as Jackson writes it."""
    f = torch.empty((records.shape[0], 37), dtype=torch.uint8, device="cuda")
    f[:, :10] = torch.frombuffer(bytearray(b'{"value":"'), dtype=torch.uint8).cuda()
    f[:, 10:34] = records
    f[:, 34:] = torch.frombuffer(bytearray(b'"},'), dtype=torch.uint8).cuda()
    t = torch.empty(37 * records.shape[0] + 1, dtype=torch.uint8, device="cuda")
    t[0] = ord("[")
    t[1:] = f.reshape(-1)
    t[-1] = ord("]")
    return t


# ---- inputs ------------------------------------------------------------------------
masked = ctx.synth_words(1, W)
tuples = ctx.synth_words(2, 2 * W).view(W, 32)
records = ctx.base64_encode_words(masked)
text = frame(records)
odos, _keep, _ = ctx.synth_odos(seed=7, n=n, words=W)
texts = [[ctx.base64_encode(f.reshape(-1)) for f in o] for o in odos]
secrets = ctx.synth_words(3, W)
torch.cuda.synchronize()
del odos, _keep

# ---- the two paths give the same bytes ---------------------------------------------
share_json, bad = ctx.convert_share_json(text, tuples, 12345, False)
words16, bad2 = ctx.base64_decode_words(records)
share_two = ctx.convert_share(words16, tuples, 12345, False)
out_text, ff, badc = ctx.mask_input_json(texts, W, secrets)
_, rec24, ff2, badc2 = ctx.mask_input_b64(texts, W, secrets, records=True)
torch.cuda.synchronize()
assert int(bad.item()) == NF and int(bad2.item()) == NF and torch.equal(share_json, share_two)
assert [int(x.item()) for x in (ff, badc, ff2, badc2)] == [NF] * 4 and torch.equal(out_text, frame(rec24))
del share_json, share_two, words16, out_text, rec24

# ---- timing: the candidates alternate -------------------------------------------------
rows = {"k_conv_json": [], "k_b64_unwords": [], "k_conv": [], "k_mask_json": [], "k_mask_b64_records": []}
for r in range(a.reps + 3):
    t_json, _ = kernel_us(lambda: ctx.convert_share_json(text, tuples, 12345, False))
    t_dec, (w16, _) = kernel_us(lambda: ctx.base64_decode_words(records))
    t_conv, _ = kernel_us(lambda: ctx.convert_share(w16, tuples, 12345, False))
    t_mj, _ = kernel_us(lambda: ctx.mask_input_json(texts, W, secrets))
    t_mb, _ = kernel_us(lambda: ctx.mask_input_b64(texts, W, secrets, records=True))
    if r >= 3:
        for k, t in zip(rows, (t_json, t_dec, t_conv, t_mj, t_mb)):
            rows[k].append(t)
rows["k_b64_unwords+k_conv"] = [x + y for x, y in zip(rows["k_b64_unwords"], rows["k_conv"])]


def stats(ts):
    q = statistics.quantiles(ts, n=4)
    return {"median_us": round(statistics.median(ts), 2), "p25_us": round(q[0], 2), "p75_us": round(q[2], 2),
            "min_us": round(min(ts), 2), "max_us": round(max(ts), 2)}


def verdict(fused, replaced):
    f, r = stats(rows[fused]), stats(rows[replaced])
    spread = r["max_us"] - r["min_us"]
    return {"fused": fused, "replaces": replaced, "ratio": round(f["median_us"] / r["median_us"], 4),
            "replaced_spread_us": round(spread, 2),
            "no_slower_beyond_spread": f["median_us"] <= r["median_us"] + spread}


bytes_per_word = {"k_conv_json": 37 + 32 + 32, "k_b64_unwords+k_conv": 24 + 16 + 16 + 32 + 32,
                  "k_mask_json": 4 * 80 * n // 3 + 16 + 37, "k_mask_b64_records": 4 * 80 * n // 3 + 16 + 24}
out = {"words": W, "parties": n, "reps": a.reps, "device": torch.cuda.get_device_name(0),
       "build_id": A._lib.build_id(),
       "kernels": {k: stats(v) for k, v in rows.items()},
       "derived_bytes_per_word": bytes_per_word,
       "GBps": {k: round(b * W / (statistics.median(rows[k]) * 1e-6) / 1e9, 1) for k, b in bytes_per_word.items()},
       "party": verdict("k_conv_json", "k_b64_unwords+k_conv"),
       "client": verdict("k_mask_json", "k_mask_b64_records")}
line = json.dumps(out)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
