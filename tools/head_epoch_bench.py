#!/usr/bin/env python3
"""Epoch time of intent-head training (BASELINE configs[4]): train_head.py's default loop (a DataLoader that unpickles one file
per utterance, pads on the host, copies from pageable memory and syncs after every step) against --device-resident (the ragged
store in HBM, batches gathered by index in the head kernels, one sync per epoch), for each pooling method.  One "epoch" is what
train_head.py does per epoch: every training batch (train_step, loss and accuracy bookkeeping) plus validation over the devel
split.  The store's one-time load (pickles -> HBM) is reported on its own.

Corpus: seeded synthetic pickles in the reference's format (sink.write_one) in a temporary directory, 11 514 train and 2 033 devel
items by default (SLURP's split sizes).  Frame counts: round(exp(N(ln 170, 0.45))) clipped to [20, 1499] (median 170 frames
= 3.4 s at 50 frames/s, mean ~ 187).  Frame values: rows of a seeded N(0, 1) pool.  The files were just written, so the default
loop reads them from the page cache: its figure is a lower bound for a cold disk.

Timing: host wall clock around whole epochs that end in a device sync; --warmup epochs first, then --repeats timed epochs
(median and min reported).  Kernel time per step: run under `rocprofv3 --kernel-trace --stats -- python tools/head_epoch_bench.py
--resident-only ...` separately.

    python tools/head_epoch_bench.py [--train-items 11514] [--devel-items 2033] [--out profiles/head_epoch_bench.json]
"""
import argparse
import importlib
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch
from torch.utils.data import DataLoader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
la = importlib.import_module("loco-asr_amd")
sink = importlib.import_module("loco-asr_amd.sink")
th = importlib.import_module("loco-asr_amd.train_head")
EmbeddingStore = importlib.import_module("loco-asr_amd.embedding_store").EmbeddingStore


def lengths_for(n, rng):
    return np.clip(np.rint(np.exp(rng.normal(np.log(170.0), 0.45, n))), 20, 1499).astype(np.int64)


def write_corpus(folder, n_train, n_devel, seed):
    rng = np.random.default_rng(seed)
    pool = rng.standard_normal((8192, 768)).astype(np.float32)
    frames = 0
    for split, n in (("train", n_train), ("devel", n_devel)):
        d = os.path.join(folder, split, "audio")
        os.makedirs(d)
        for i, T in enumerate(lengths_for(n, rng)):
            start = int(rng.integers(0, pool.shape[0] - T + 1))
            tgt = np.zeros(101, dtype=np.int64)
            tgt[int(rng.integers(0, 101))] = 1
            sink.write_one(d, f"{split}{i:06d}", pool[start:start + T], tgt)
            frames += int(T)
    return frames


def epoch_default(model, train_set, val_set, g, device):
    """train_head.main's default epoch body (W = 1) + evaluate()"""
    ids, mine = th.epoch_batches(len(train_set), 16, 1, 0, g)
    loader = DataLoader(train_set, batch_sampler=mine, collate_fn=th.collate_fn)
    epoch_loss, acc, n = 0.0, 0.0, 0
    for i, (_, data, target) in zip(ids, loader):
        loss, pred = model.train_step(data.to(device), target.to(device))
        epoch_loss += float(loss)
        acc += float((pred.argmax(1) == target.to(device).argmax(1)).float().sum())
        n += 1
    val_loader = DataLoader(val_set, batch_sampler=th.strided_batches(len(val_set), 16, 1, 0), collate_fn=th.collate_fn)
    vl, va = th.evaluate(model, val_loader, device, len(val_set))
    return n, epoch_loss / n, vl


def epoch_resident(model, train_store, val_store, val_plan, g, device):
    """train_head.main's --device-resident epoch body (W = 1) + evaluate_resident()"""
    ids, mine = th.epoch_batches(len(train_store), 16, 1, 0, g)
    loss_sum = torch.zeros((), dtype=torch.float64, device=device)
    correct = torch.zeros((), dtype=torch.int64, device=device)
    n = 0
    for i, (idx, T_pad) in zip(ids, train_store.batches(mine)):
        loss, pred = model.train_step_ragged(train_store, idx, T_pad)
        loss_sum += loss.double()
        correct += (pred.argmax(1) == train_store.targets[idx].argmax(1)).sum()
        n += 1
    vl, va = th.evaluate_resident(model, val_store, val_plan, device, len(val_store))
    return n, float(loss_sum) / n, vl


def timed(fn, warmup, repeats):
    out, times = None, []
    for r in range(warmup + repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if r >= warmup:
            times.append(time.perf_counter() - t0)
    return times, out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--train-items", type=int, default=11514)
    ap.add_argument("--devel-items", type=int, default=2033)
    ap.add_argument("--methods", default="average,max,attention")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--tmpdir", default=None, help="where the pickle corpus is written (default: the system temp dir)")
    ap.add_argument("--resident-only", action="store_true", help="skip the default loop (for a rocprofv3 kernel-trace run)")
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a ROCm device")
    device = torch.device("cuda", 0)
    tmp = tempfile.mkdtemp(prefix="head_epoch_bench_", dir=args.tmpdir)
    try:
        est = int(np.exp(np.log(170.0) + 0.45 ** 2 / 2) * 768 * 4 * (args.train_items + args.devel_items) * 1.05)
        free = shutil.disk_usage(tmp).free
        if est > free:
            raise SystemExit(f"the corpus needs about {est} bytes in {tmp}, {free} free: pass --tmpdir or fewer items")
        t0 = time.perf_counter()
        frames = write_corpus(tmp, args.train_items, args.devel_items, args.seed)
        t_write = time.perf_counter() - t0
        print(f"corpus: {args.train_items} train + {args.devel_items} devel pickles, {frames} frames "
              f"({frames * 3072 / 1e9:.2f} GB), written in {t_write:.1f} s", flush=True)
        train_set = sink.EmbeddingsTargets(tmp, "audio", "train")
        val_set = sink.EmbeddingsTargets(tmp, "audio", "devel")
        t0 = time.perf_counter()
        train_store = EmbeddingStore.from_folders(tmp, "audio", ["train"], device)
        val_store = EmbeddingStore.from_folders(tmp, "audio", ["devel"], device)
        torch.cuda.synchronize()
        t_load = time.perf_counter() - t0
        print(f"store load (once per run): {t_load:.2f} s for {train_store.nbytes + val_store.nbytes} bytes", flush=True)
        val_plan = val_store.batches(th.strided_batches(len(val_store), 16, 1, 0))
        res = {"corpus": {"train_items": args.train_items, "devel_items": args.devel_items, "frames": frames,
                          "lengths": "round(exp(N(ln 170, 0.45))) clipped to [20, 1499] frames",
                          "train_frames_mean": float(train_store.lengths.mean()), "train_frames_max": int(train_store.lengths.max()),
                          "bytes_in_hbm": train_store.nbytes + val_store.nbytes, "page_cache": "warm (just written)"},
               "store_load_s": round(t_load, 3), "warmup": args.warmup, "repeats": args.repeats,
               "device": torch.cuda.get_device_name(device), "methods": {}}
        for method in args.methods.split(","):
            row = {}
            torch.manual_seed(0)
            model = la.IntentClassifierMI355X(method).to(device)
            if not args.resident_only:
                g = torch.Generator().manual_seed(0)
                times, (n, tl, vl) = timed(lambda: epoch_default(model, train_set, val_set, g, device), args.warmup, args.repeats)
                row["default_epoch_s"] = {"median": round(statistics.median(times), 4), "min": round(min(times), 4),
                                          "all": [round(t, 4) for t in times]}
                print(f"{method:9s} default loop:    epoch + validation {statistics.median(times):8.3f} s  ({n} steps)", flush=True)
            torch.manual_seed(0)
            model = la.IntentClassifierMI355X(method).to(device)
            g = torch.Generator().manual_seed(0)
            times, (n, tl, vl) = timed(lambda: epoch_resident(model, train_store, val_store, val_plan, g, device), args.warmup,
                                       args.repeats)
            row["resident_epoch_s"] = {"median": round(statistics.median(times), 4), "min": round(min(times), 4),
                                       "all": [round(t, 4) for t in times]}
            row["steps_per_epoch"] = n
            row["resident_ms_per_step_incl_validation"] = round(1e3 * statistics.median(times) / n, 4)
            msg = f"{method:9s} device-resident: epoch + validation {statistics.median(times):8.3f} s  ({n} steps)"
            if "default_epoch_s" in row:
                row["speedup"] = round(row["default_epoch_s"]["median"] / row["resident_epoch_s"]["median"], 2)
                msg += f"  speed-up x{row['speedup']}"
            print(msg, flush=True)
            res["methods"][method] = row
        line = json.dumps(res)
        print(line)
        if args.out:
            with open(args.out, "w") as fh:
                fh.write(json.dumps(res, indent=1) + "\n")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
