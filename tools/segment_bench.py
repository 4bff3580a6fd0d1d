#!/usr/bin/env python3
"""What cutting a recording costs next to encoding it -> profiles/segment_cost.json (tools, not bench.py): the frame-energy kernel and
the segmentation kernel on a synthetic 60-minute recording (57.6 M samples, F = 179 999), and the encoder forward of the recording's
first 10-minute window in the same process.  Warm-up first, medians of --reps runs, timed with events on the stream."""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
la = importlib.import_module("loco-asr_amd")
seg = importlib.import_module("loco-asr_amd.segment")


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


def recording(samples, seed=0):
    """Speech-like gating on the device: runs of 0.05-amplitude noise (mean 3 s) between pauses of 1e-4 noise (mean 0.6 s)."""
    rng = np.random.default_rng(seed)
    frames = samples // seg.HOP + 1
    gate, t, on = np.empty(frames, np.float32), 0, True
    while t < frames:
        n = int(rng.geometric(1.0 / (150 if on else 30)))
        gate[t:t + n] = 0.05 if on else 1e-4
        t, on = t + n, not on
    g = torch.Generator(device="cuda").manual_seed(seed)
    env = torch.from_numpy(gate).cuda().repeat_interleave(seg.HOP)[:samples]
    return env * torch.randn(samples, device="cuda", generator=g)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--minutes", type=float, default=60.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segment_cost.json"))
    args = ap.parse_args()
    n = int(args.minutes * 60 * seg.SAMPLE_RATE)
    wave = recording(n)
    params = seg.resolve_params(None)
    db = seg.frame_energy_db(wave)
    res = {"clock_state": "as found (not pinned)", "reps": args.reps, "samples": n, "frames": int(db.shape[0])}
    res["frame_energy_ms"] = timed(lambda: seg.frame_energy_db(wave), args.reps)
    res["vad_segments_ms"] = timed(lambda: seg.segments_from_db(db, params), args.reps)  # allocates its outputs and workspace, as segment() does
    s = seg.segment(wave)
    lengths = (s.end_frames - s.start_frames).cpu().numpy()
    res["segments"] = s.count
    res["threshold_db"] = s.threshold_db
    res["segment_frames_mean_max"] = [float(lengths.mean()), int(lengths.max())]
    print(res, flush=True)

    t = lambda d: {k: torch.from_numpy(v) for k, v in d.items()}  # noqa: E731
    pre, enc = la.synth.split_state_dict(la.synth.encoder_state_dict(0))
    model = la.SpeechT5ForSpeechToTextMI355X.from_state_dicts(t(pre), t(enc)).to("cuda")
    window = wave[:min(n, 600 * seg.SAMPLE_RATE)][None].contiguous()
    mask = torch.ones(window.shape, dtype=torch.int32, device="cuda")
    encode = lambda: model.speecht5.encoder(input_values=window, attention_mask=mask)  # noqa: E731
    res["encoder_window_samples"] = int(window.shape[1])
    res["encoder_window_ms"] = timed(encode, max(3, args.reps // 3), warmup=1)
    windows = n / window.shape[1]
    res["cutting_over_encoding_of_the_whole_recording"] = (res["frame_energy_ms"] + res["vad_segments_ms"]) / (res["encoder_window_ms"] * windows)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
