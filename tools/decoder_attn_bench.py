#!/usr/bin/env python3
"""What the decoder's attention probabilities and token timestamps cost -> profiles/decoder_attn_cost.json (tools, not bench.py): the
teacher-forced decoder pass with and without output_attentions, and align, each at B = 8, S = 100, T_enc = 249 and at B = 4, S = 450,
T_enc = 1499, next to the store-byte floor of the P they write.  Warm-up first, medians of --reps runs, timed with events on the stream."""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
la = importlib.import_module("loco-asr_amd")

COPY_RATE = 6.29e12  # bytes/s: the part's measured float4 copy bandwidth; a store-only kernel moves half a copy's bytes per byte stored


def timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decoder_attn_cost.json"))
    args = ap.parse_args()
    t = lambda d: {k: torch.from_numpy(v) for k, v in d.items()}  # noqa: E731
    pre, enc = la.synth.split_state_dict(la.synth.encoder_state_dict(0))
    dec, post = la.synth.split_decoder_state_dict(la.synth.decoder_state_dict(0))
    model = la.SpeechT5ForSpeechToTextMI355X.from_state_dicts(t(pre), t(enc), decoder_state_dict=t(dec), postnet_state_dict=t(post)).to("cuda")
    x, m = la.synth.batch([16000, 16000])
    model.generate(torch.from_numpy(x).cuda(), torch.from_numpy(m).cuda(), max_length=4)  # loads the weights
    rt = model._decoder_runtime
    res = {"clock_state": "as found (not pinned)", "reps": args.reps, "copy_rate_bytes_per_s": COPY_RATE, "grid": []}
    for B, S, T in ((8, 100, 249), (4, 450, 1499)):
        enc_out = torch.randn((B, T, 768), device="cuda")
        ids = torch.randint(4, 81, (B, S), dtype=torch.int32, device="cuda")
        counts = torch.full((B,), S, dtype=torch.int32, device="cuda")
        row = dict(B=B, S=S, T_enc=T)
        row["forward_ms"] = timed(lambda: rt.forward(enc_out, None, ids), args.reps)
        row["forward_attn_ms"] = timed(lambda: rt.forward_attn(enc_out, None, ids), args.reps)  # allocates its 12 output tensors, as the model's call does
        row["align_ms"] = timed(lambda: rt.align(enc_out, None, ids, counts), args.reps)
        p_bytes = 4.0 * 6 * B * 12 * S * (S + T)
        row["P_bytes_forward_attn"] = p_bytes
        row["store_floor_forward_attn_ms"] = p_bytes / COPY_RATE * 1e3
        row["attn_extra_over_store_floor"] = (row["forward_attn_ms"] - row["forward_ms"]) / row["store_floor_forward_attn_ms"]
        cross = 4.0 * 6 * B * 12 * S * T
        row["P_bytes_align"] = cross  # written once and read once by the mean, one layer at a time
        row["store_floor_align_ms"] = 2 * cross / COPY_RATE * 1e3
        res["grid"].append(row)
        print(row, flush=True)
        del enc_out
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
