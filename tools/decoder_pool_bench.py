#!/usr/bin/env python3
"""Corpus transcription timings -> profiles/decoder_pool.json (tools, not bench.py).  A synthetic corpus of --utterances clips of 2-6 s
in the reference's pairs, caps from a fixed-seed long-tailed distribution (90 % in 10-60, 10 % at 450), all 6 decoder layers, one
process, every variant timed --reps times in alternation (wall clock around a synchronised call, encoder included):
  (i)   generate per pair, max_length = the pair's larger cap: the loop transcribe.py runs without --slots
  (ii)  generate on 64 packed rows (32 pairs through forward_packed), max_length = the group's largest cap, no refill
  (iii) generate_many: the pool at 64 slots
Tokens are the tokens an utterance asked for (up to its own cap or </s>), the same count in every variant.  Then one guard against a
regression inside the feature: a pool step with 64 open slots at T_enc = 249 against loco_decoder_step at B = 64 and the same T_enc,
three alternated runs each, next to the spread of loco_decoder_step's own three runs.  The encoder rows are drawn so that all 64 slots
are still open after the timed steps (the poll block is read after every run).  Exits 1 when the pool's best step is slower than
loco_decoder_step's best by more than that spread, or when a slot closed during a timed run."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
la = importlib.import_module("loco-asr_amd")
_libmod = importlib.import_module("loco-asr_amd._lib")
dec = importlib.import_module("loco-asr_amd.decoder")


def corpus(n, seed=5):
    rng = np.random.Generator(np.random.Philox(seed))
    lengths = [int(16000 * (2.0 + 4.0 * u)) for u in rng.random(n)]
    caps = [450 if u < 0.10 else 10 + int(51 * v) for u, v in zip(rng.random(n), rng.random(n))]
    batches = []
    for b0 in range(0, n, 2):
        x, m = la.synth.batch(lengths[b0:b0 + 2], first_index=b0)
        batches.append(dict(input_values=torch.from_numpy(x).cuda(), attention_mask=torch.from_numpy(m).cuda()))
    return batches, caps


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decoder_pool.json"))
    args = ap.parse_args()
    t = lambda d: {k: torch.from_numpy(v) for k, v in d.items()}  # noqa: E731
    pre, enc = la.synth.split_state_dict(la.synth.encoder_state_dict(0))
    dsd, post = la.synth.split_decoder_state_dict(la.synth.decoder_state_dict(0))
    model = la.SpeechT5ForSpeechToTextMI355X.from_state_dicts(t(pre), t(enc), decoder_state_dict=t(dsd), postnet_state_dict=t(post)).to("cuda")
    lib, e, rt = _libmod.load(), model.speecht5.encoder, model._decoder_runtime
    batches, caps = corpus(args.utterances)
    model.generate(**batches[0], max_length=8)  # loads the weights

    def per_pair():
        n = 0
        for k, b in enumerate(batches):
            model.generate(**b, max_length=max(caps[2 * k:2 * k + 2]))
            n += sum(min(int(v), c) - 1 for v, c in zip(rt.last_lengths.tolist(), caps[2 * k:2 * k + 2]))
        return n

    def packed64():
        n = 0
        for g0 in range(0, len(batches), 32):
            ticket = e.forward_packed_async(batches[g0:g0 + 32])
            ticket.result()
            out, _ = ticket.packed_output()
            cs = caps[2 * g0:2 * g0 + out.shape[0]]
            rt.generate(out, e.last_frames, max(cs), False)
            n += sum(min(int(v), c) - 1 for v, c in zip(rt.last_lengths.tolist(), cs))
        return n

    def pool64():
        return sum(len(r) - 1 for r in model.generate_many(batches, max_length=caps, slots=64, pack=32))

    variants = {"generate_per_pair": per_pair, "generate_64_rows_no_refill": packed64, "pool_64_slots": pool64}
    runs = {k: [] for k in variants}
    tokens = {}
    for _ in range(args.reps):
        for k, fn in variants.items():
            s, n = wall(fn)
            runs[k].append(s)
            tokens[k] = n
            print(k, f"{s:.3f} s, {n} tokens", flush=True)
    res = {"clock_state": "as found (not pinned)", "utterances": args.utterances, "reps": args.reps, "caps": "90 % in 10-60, 10 % at 450, Philox seed 5",
           "variants": {k: dict(seconds=v, tokens=tokens[k], tokens_per_s=tokens[k] / min(v), utterances_per_s=args.utterances / min(v))
                        for k, v in runs.items()}}
    # the step guard
    B, T, S = 64, 249, 450
    p = lambda tn: C.c_void_p(tn.data_ptr())  # noqa: E731
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    need = int(lib.loco_decoder_workspace_bytes(e._handle, B, T, S))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    pneed = int(lib.loco_decoder_pool_workspace_bytes(e._handle, B, T, S))
    pws = torch.empty(pneed, dtype=torch.uint8, device="cuda")
    ids, rows, cps = (C.c_int32 * B)(*range(B)), (C.c_int32 * B)(*[T] * B), (C.c_int32 * B)(*[S] * B)

    block = torch.zeros(4 + 2 * B, dtype=torch.int32).pin_memory()

    def still_open():
        _libmod.check(lib.loco_decoder_pool_poll(e._handle, B, T, S, p(block), p(pws), pneed, st()))
        torch.cuda.synchronize()
        return int(block[0])

    def parent_steps():
        _libmod.check(lib.loco_decoder_begin(e._handle, p(enc_out), None, B, T, S, p(ws), need, st()))
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(args.steps):
            _libmod.check(lib.loco_decoder_step(e._handle, B, T, S, i, None, p(ws), need, st()))
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / args.steps

    def pool_steps():
        _libmod.check(lib.loco_decoder_pool_init(e._handle, B, T, S, p(pws), pneed, st()))
        _libmod.check(lib.loco_decoder_pool_admit(e._handle, B, T, S, B, ids, p(enc_out), T * 768, rows, None, cps, p(pws), pneed, st()))
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(args.steps):
            _libmod.check(lib.loco_decoder_pool_step(e._handle, B, T, S, i, T, None, p(pws), pneed, st()))
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / args.steps

    # with synthetic weights a row ends at its first token or never: draw encoder rows until every slot outlives the timed steps
    for seed in range(16):
        enc_out = torch.randn((B, T, 768), device="cuda", generator=torch.Generator("cuda").manual_seed(seed))
        pool_steps()
        if still_open() == B:
            break
    else:
        sys.exit("no draw of encoder rows keeps all 64 slots open")
    parent_steps()  # warm-up
    ps, qs, opens = [], [], []
    for _ in range(3):
        ps.append(parent_steps())
        qs.append(pool_steps())
        opens.append(still_open())
    ok = min(qs) - min(ps) <= max(ps) - min(ps) and opens == [B] * 3
    res["step_B64_T249"] = dict(decoder_step_ms=ps, pool_step_ms=qs, decoder_step_spread_ms=max(ps) - min(ps), encoder_rows_seed=seed,
                                pool_minus_decoder_ms=min(qs) - min(ps), slots_open_after_each_run=opens, within_spread=bool(ok))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
