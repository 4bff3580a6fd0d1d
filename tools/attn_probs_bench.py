#!/usr/bin/env python3
"""Cost of output_attentions=True: the speech encoder's forward (synthetic weights, precision f16x3 by default) at 30 s x 8 and
30 s x 32, with and without the attention probabilities, timed with device events after warm-up.  The probabilities are
layers * B * 12 * T^2 * 4 bytes (30 s x 32: 41 GB), allocated by each call as the encoder does.

The attention_probs kernel's own time comes from a separate run under
`rocprofv3 --kernel-trace --stats -- python tools/attn_probs_bench.py --attn-only`; bytes written / kernel time is then the
kernel's store rate (the MI355X plain-store figure for this shape: 6.0-6.2 TB/s).

    python tools/attn_probs_bench.py [--batches 8 32] [--repeats 5] [--precision f16x3] [--out profiles/attn_probs_bench.txt]
"""
import argparse
import importlib
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
la = importlib.import_module("loco-asr_amd")


def build(precision):
    sd = la.synth.encoder_state_dict(0)
    pre, enc = la.synth.split_state_dict(sd)
    m = la.SpeechT5ForSpeechToTextMI355X.from_state_dicts({k: torch.from_numpy(v) for k, v in pre.items()},
                                                          {k: torch.from_numpy(v) for k, v in enc.items()}, precision=precision)
    return m.to("cuda").speecht5.encoder


def time_forward(enc, x, m, attn, warmup, repeats):
    for _ in range(warmup):
        out = enc(input_values=x, attention_mask=m, output_attentions=attn)
        del out
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = enc(input_values=x, attention_mask=m, output_attentions=attn)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
        del out
    return statistics.median(times), min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--precision", default="f16x3")
    ap.add_argument("--attn-only", action="store_true", help="only the forwards with output_attentions (for the kernel trace)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    enc = build(args.precision)
    lines = [f"attn_probs_bench: precision {args.precision}, {torch.cuda.get_device_name()}, median / min of {args.repeats} after "
             f"{args.warmup} warm-up forwards, device events around the whole call"]
    for B in args.batches:
        x, m = la.synth.batch([480000] * B)
        x, m = torch.from_numpy(x).cuda(), torch.from_numpy(m).cuda()
        T = int(importlib.import_module("loco-asr_amd._lib").load().loco_output_frames(480000))
        gb = 12 * B * 12 * T * T * 4 / 1e9
        with torch.no_grad():
            if not args.attn_only:
                med0, min0 = time_forward(enc, x, m, False, args.warmup, args.repeats)
                lines.append(f"30 s x {B:2d}  default forward            median {med0:9.2f} ms  min {min0:9.2f} ms")
            med1, min1 = time_forward(enc, x, m, True, args.warmup, args.repeats)
            lines.append(f"30 s x {B:2d}  output_attentions=True     median {med1:9.2f} ms  min {min1:9.2f} ms  ({gb:.1f} GB of probabilities)")
            if not args.attn_only:
                lines.append(f"30 s x {B:2d}  difference                 median {med1 - med0:9.2f} ms  -> {gb / ((med1 - med0) / 1e3):.0f} "
                             f"GB/s of probabilities per second of extra time")
        print(lines[-1] if args.attn_only else "\n".join(lines[-3:]), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
