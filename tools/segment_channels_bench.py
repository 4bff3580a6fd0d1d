#!/usr/bin/env python3
"""What cutting a two-channel recording per channel costs next to cutting its channels one by one -> profiles/segment_channels_cost.json
(tools, not bench.py): on a synthetic two-channel 10-minute and 60-minute call, the batched energy kernel, the per-channel segmentation
kernel and the overlap kernel, against two mono ``frame_energy_db`` + ``segments_from_db`` calls in the same process.  Warm-up first,
medians of --reps runs, timed with events on the stream.  There is no bar: the figures are recorded."""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
seg = importlib.import_module("loco-asr_amd.segment")
from segment_bench import recording, timed  # noqa: E402


def call(samples, leak_db=-20.0):
    """f32 [2, samples]: two independent speech-like channels (segment_bench.recording), each carrying the other at leak_db."""
    a, b = recording(samples, seed=1), recording(samples, seed=2)
    g = 10.0 ** (leak_db / 20.0)
    return torch.stack([a + g * b, b + g * a]).contiguous()


def measure(minutes, reps, crosstalk_db):
    n = int(minutes * 60 * seg.SAMPLE_RATE)
    waves = call(n)
    params = seg.resolve_params(None)
    db = seg.frame_energy_db_channels(waves)
    res = {"minutes": minutes, "samples": n, "frames": int(db.shape[1]), "channels": 2, "crosstalk_db": crosstalk_db}
    res["energy_channels_ms"] = timed(lambda: seg.frame_energy_db_channels(waves), reps)
    res["segments_channels_ms"] = timed(lambda: seg.segments_channels_from_db(db, params, crosstalk_db, overlap=False), reps)
    res["segments_channels_with_overlap_ms"] = timed(lambda: seg.segments_channels_from_db(db, params, crosstalk_db), reps)
    res["overlap_ms"] = res["segments_channels_with_overlap_ms"] - res["segments_channels_ms"]
    res["two_mono_energy_ms"] = timed(lambda: [seg.frame_energy_db(waves[c]) for c in range(2)], reps)
    res["two_mono_segments_ms"] = timed(lambda: [seg.segments_from_db(db[c], params) for c in range(2)], reps)
    split = res["energy_channels_ms"] + res["segments_channels_with_overlap_ms"]
    mono = res["two_mono_energy_ms"] + res["two_mono_segments_ms"]
    res["split_total_ms"], res["two_mono_total_ms"], res["split_over_two_mono"] = split, mono, split / mono
    s = seg.segment_channels(waves, crosstalk_db)
    res["segments_per_channel"] = s.counts
    res["threshold_db"] = s.threshold_db
    res["overlap_frames_total"] = int(s.overlap_frames.sum().item())
    plain = seg.segment_channels(waves, float("inf"))
    res["segments_per_channel_without_gate"] = plain.counts
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--minutes", type=float, nargs="+", default=[10.0, 60.0])
    ap.add_argument("--crosstalk-db", type=float, default=seg.DEFAULT_CROSSTALK_DB)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segment_channels_cost.json"))
    args = ap.parse_args()
    res = {"clock_state": "as found (not pinned)", "reps": args.reps, "recordings": []}
    for minutes in args.minutes:
        res["recordings"].append(measure(minutes, args.reps, args.crosstalk_db))
        print(res["recordings"][-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
