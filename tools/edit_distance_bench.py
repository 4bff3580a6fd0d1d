#!/usr/bin/env python3
"""What the device-side edit distance costs -> profiles/edit_distance_cost.json (a tool, not bench.py; no figure is fixed in advance:
nothing exists at the parent commit to compare with, the file records what was measured).

    python tools/edit_distance_bench.py [--reps 9] [--utterances 512] [--nbest 16] [--no-model]

1. loco_op_edit_distance alone, on packed device buffers, device events around one launch, warm-up, median of --reps:
   a. 4 096 pairs of 60 - 140 symbols a side (alphabet 81, hypotheses a fifth redrawn), max_len 256;
   b. the MBR shape: --utterances lists of --nbest hypotheses of 60 - 140 symbols, all N (N - 1) / 2 pairs of every list in one launch,
      and loco_op_nbest_risk on its counts;
   c. one 16 384 x 16 384 pair (the one-wave-per-workgroup form).
   Reported: milliseconds, pairs / s and cell updates / s (cells = ref_len * hyp_len summed over the pairs).
2. The same through metrics.edit_counts / metrics.mbr_select from host sequences (packing, upload, bucketed launches, one read-back):
   host clock around synchronised work.
3. The numpy restatement (tests/edit_distance_ref.py) on the host, one thread, on a sample of a. (and once on a 2 048 x 2 048 pair):
   pairs / s and cells / s beside the core count the process may use.
4. Unless --no-model: sample_many at N = --nbest on the --utterances corpus of tools/decoder_pool_bench.py (full synthetic weights),
   once, then mbr_select on its hypotheses: the share of MBR in an n-best pass.
Clocks as found (not pinned); one process, one device."""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def make_pairs(rng, count, lo=60, hi=140, k=81):
    refs, hyps = [], []
    for _ in range(count):
        a = rng.integers(3, 3 + k, rng.integers(lo, hi + 1))
        b = np.resize(a, rng.integers(lo, hi + 1))
        hyps.append(np.where(rng.random(b.size) < 0.2, rng.integers(3, 3 + k, b.size), b).astype(np.int64))
        refs.append(a.astype(np.int64))
    return refs, hyps


def pack(seqs):
    lens = np.array([len(s) for s in seqs], dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    return np.concatenate(seqs).astype(np.int32), starts, lens


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--utterances", type=int, default=512)
    ap.add_argument("--nbest", type=int, default=16)
    ap.add_argument("--no-model", action="store_true", help="skip 4. (sample_many on the full synthetic model)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit_distance_cost.json"))
    args = ap.parse_args()
    import torch
    la = importlib.import_module("loco-asr_amd")
    _libmod = importlib.import_module("loco-asr_amd._lib")
    metrics = la.metrics
    import edit_distance_ref as ref
    lib = _libmod.load()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731

    def events(fn):
        """Median, min and max milliseconds of --reps runs of fn between device events, after two warm-up runs."""
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), reps=args.reps)

    def wall(fn):
        fn()
        torch.cuda.synchronize()
        s = []
        for _ in range(min(args.reps, 5)):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            s.append(time.perf_counter() - t0)
        return dict(median_ms=1e3 * statistics.median(s), min_ms=1e3 * min(s), max_ms=1e3 * max(s), reps=len(s))

    def rates(entry, pairs, cells):
        s = entry["median_ms"] * 1e-3
        entry.update(pairs=int(pairs), cells=int(cells), pairs_per_s=pairs / s, cell_updates_per_s=cells / s)
        return entry

    def kernel_case(symbols, spans, max_len):
        sym = torch.from_numpy(symbols).cuda()
        sp = torch.from_numpy(np.ascontiguousarray(spans, dtype=np.int32)).cuda()
        out = torch.empty((sp.shape[0], 4), dtype=torch.int32, device="cuda")
        fn = lambda: _libmod.check(lib.loco_op_edit_distance(p(sym), sym.numel(), p(sp), sp.shape[0], max_len, p(out), st()))  # noqa: E731
        e = rates(events(fn), sp.shape[0], int((spans[:, 1].astype(np.int64) * spans[:, 3]).sum()))
        assert int(out.min()) >= 0
        return e, out

    rng = np.random.default_rng(5)
    res = {"clock_state": "as found (not pinned)", "device": torch.cuda.get_device_name(0),
           "host_cores_usable": len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()}

    # a. 4 096 pairs
    refs, hyps = make_pairs(rng, 4096)
    sym, starts, lens = pack(refs + hyps)
    spans = np.stack([starts[:4096], lens[:4096], starts[4096:], lens[4096:]], axis=1)
    res["pairs_4096_len_60_140"] = {"kernel": kernel_case(sym, spans, 256)[0],
                                    "metrics_edit_counts_from_host": rates(wall(lambda: metrics.edit_counts(refs, hyps)), 4096,
                                                                           int((lens[:4096] * lens[4096:]).sum()))}
    print(json.dumps(res["pairs_4096_len_60_140"]), flush=True)

    # b. the MBR shape
    U, N = args.utterances, args.nbest
    lists = []
    for _ in range(U):
        base, per = make_pairs(rng, 1)[0][0], []
        for _ in range(N):
            b = np.resize(base, rng.integers(60, 141))
            per.append(np.where(rng.random(b.size) < 0.2, rng.integers(3, 84, b.size), b).astype(np.int64))
        lists.append(per)
    flat = [h for per in lists for h in per]
    sym, starts, lens = pack(flat)
    i, j = np.triu_indices(N, k=1)
    left = (np.arange(U)[:, None] * N + i[None, :]).ravel()
    right = (np.arange(U)[:, None] * N + j[None, :]).ravel()
    spans = np.stack([starts[left], lens[left], starts[right], lens[right]], axis=1)
    e, counts = kernel_case(sym, spans, 256)
    offs = torch.arange(0, U * N + 1, N, dtype=torch.int32, device="cuda")
    risk = torch.empty(U * N, dtype=torch.float64, device="cuda")
    best = torch.empty(U, dtype=torch.int32, device="cuda")
    r = events(lambda: _libmod.check(lib.loco_op_nbest_risk(p(counts), p(offs), None, U, p(risk), p(best), st())))
    res["mbr_shape"] = {"utterances": U, "nbest": N, "edit_distance_kernel": e, "nbest_risk_kernel": r,
                        "metrics_mbr_select_from_host": rates(wall(lambda: metrics.mbr_select(lists)), spans.shape[0],
                                                              int((spans[:, 1] * spans[:, 3]).sum()))}
    print(json.dumps(res["mbr_shape"]), flush=True)

    # c. one pair at the cap
    cap = metrics.max_len()
    a = rng.integers(0, 4, cap)
    b = np.where(rng.random(cap) < 0.2, rng.integers(0, 4, cap), a)
    sym = np.concatenate([a, b]).astype(np.int32)
    res["one_pair_16384_x_16384"] = {"kernel": kernel_case(sym, np.array([[0, cap, cap, cap]], dtype=np.int64), cap)[0]}
    print(json.dumps(res["one_pair_16384_x_16384"]), flush=True)

    # 3. the numpy restatement on the host
    sample = 64
    t0 = time.perf_counter()
    for a_, b_ in zip(refs[:sample], hyps[:sample]):
        ref.edit_counts(a_, b_)
    s = time.perf_counter() - t0
    cells = int(sum(len(a_) * len(b_) for a_, b_ in zip(refs[:sample], hyps[:sample])))
    big = 2048
    t0 = time.perf_counter()
    ref.edit_counts(a[:big], b[:big])
    s_big = time.perf_counter() - t0
    res["numpy_restatement_host"] = {"threads": 1, "host_cores_usable": res["host_cores_usable"],
                                     "pairs_len_60_140": dict(pairs=sample, seconds=s, pairs_per_s=sample / s, cell_updates_per_s=cells / s),
                                     "one_pair_2048_x_2048": dict(seconds=s_big, cell_updates_per_s=big * big / s_big)}
    print(json.dumps(res["numpy_restatement_host"]), flush=True)

    # 4. the share of MBR in an n-best pass
    if not args.no_model:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        from decoder_pool_bench import corpus
        t = lambda d: {k: torch.from_numpy(v) for k, v in d.items()}  # noqa: E731
        pre, enc = la.synth.split_state_dict(la.synth.encoder_state_dict(0))
        dsd, post = la.synth.split_decoder_state_dict(la.synth.decoder_state_dict(0))
        model = la.SpeechT5ForSpeechToTextMI355X.from_state_dicts(t(pre), t(enc), decoder_state_dict=t(dsd), postnet_state_dict=t(post)).to("cuda")
        batches, caps = corpus(U)
        model.generate(**batches[0], max_length=8)  # loads the weights
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hyps_m = model.sample_many(batches, num_return_sequences=N, temperature=0.8, top_p=0.95, seed=5, max_length=caps, slots=64, pack=32)
        torch.cuda.synchronize()
        s_sample = time.perf_counter() - t0
        m = wall(lambda: metrics.mbr_select(hyps_m))
        tokens = sum(len(h) - 1 for per in hyps_m for h in per)
        res["nbest_pass"] = {"utterances": U, "nbest": N, "caps": "90 % in 10-60, 10 % at 450, Philox seed 5", "sample_many_s": s_sample,
                             "sample_many_runs": 1, "tokens": tokens, "mbr_select": m,
                             "mbr_share_of_the_pass": m["median_ms"] * 1e-3 / (s_sample + m["median_ms"] * 1e-3)}
        print(json.dumps(res["nbest_pass"]), flush=True)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
