#!/usr/bin/env python3
"""What beam search in the slot pool costs -> profiles/decoder_beam_cost.json (tools, not bench.py; it sets no bar).  All 6 decoder
layers, one process, device events, the median of 9, clocks as found.
  (i)   one step of a pool of 64 slots at T_enc = 249: loco_decoder_pool_step (greedy, 64 utterances) against
        loco_decoder_pool_step_beam with K = 4 (16 groups) and K = 16 (4 groups), runs of --steps steps from admission, alternated
  (ii)  the reorder's share: a beam pool (K = 4) stepped from admission to position 404, every step timed; at positions 10, 100 and 400
        the median of the 9 steps around it, how many slots changed parent there, and loco_op_beam_reorder alone on buffers of the
        pool's shape with EVERY slot changing parent (a rotation inside each group) and count = position + 1 -- the most it can move
  (iii) tokens/s of beam_search_many (K = 4, the best hypothesis' tokens) against generate_many on tools/decoder_pool_bench.py's
        512-utterance set, wall clock around a synchronised call, encoder included
The encoder rows of (i) and (ii) are drawn so that every slot is still open after the timed steps."""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
la = importlib.import_module("loco-asr_amd")
_libmod = importlib.import_module("loco-asr_amd._lib")
dec = importlib.import_module("loco-asr_amd.decoder")
from decoder_pool_bench import corpus  # noqa: E402

B, T, S = 64, 249, 450
p = lambda tn: C.c_void_p(tn.data_ptr()) if tn is not None else None  # noqa: E731
st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=512)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decoder_beam_cost.json"))
    args = ap.parse_args()
    t = lambda d: {k: torch.from_numpy(v) for k, v in d.items()}  # noqa: E731
    pre, enc = la.synth.split_state_dict(la.synth.encoder_state_dict(0))
    dsd, post = la.synth.split_decoder_state_dict(la.synth.decoder_state_dict(0))
    model = la.SpeechT5ForSpeechToTextMI355X.from_state_dicts(t(pre), t(enc), decoder_state_dict=t(dsd), postnet_state_dict=t(post)).to("cuda")
    lib, e = _libmod.load(), model.speecht5.encoder
    batches, caps = corpus(args.utterances)
    model.generate(**batches[0], max_length=8)  # loads the weights
    layers = e._decoder_layers
    res = {"clock_state": "as found (not pinned)", "slots": B, "T_enc": T, "S_max": S, "median_of": 9}
    block = torch.zeros(4 + 2 * B, dtype=torch.int32).pin_memory()
    i32 = lambda vs: (C.c_int32 * len(vs))(*vs)  # noqa: E731

    def open_slots(ws):
        _libmod.check(lib.loco_decoder_pool_poll(e._handle, B, T, S, p(block), p(ws), ws.numel(), st()))
        torch.cuda.synchronize()
        return int(block[0])

    gws = torch.empty(int(lib.loco_decoder_pool_workspace_bytes(e._handle, B, T, S)), dtype=torch.uint8, device="cuda")

    def greedy_run(enc_out, steps):
        _libmod.check(lib.loco_decoder_pool_init(e._handle, B, T, S, p(gws), gws.numel(), st()))
        _libmod.check(lib.loco_decoder_pool_admit(e._handle, B, T, S, B, i32(range(B)), p(enc_out), T * 768, i32([T] * B), None, i32([S] * B), p(gws),
                                                  gws.numel(), st()))
        torch.cuda.synchronize()
        return timed(lambda: [_libmod.check(lib.loco_decoder_pool_step(e._handle, B, T, S, i, T, None, p(gws), gws.numel(), st())) for i in range(steps)]) / steps

    def beam_pool(K):
        cfg = dec.check_beam_args(K)[2]
        ws = torch.empty(int(lib.loco_decoder_beam_workspace_bytes(e._handle, B, T, S, K)), dtype=torch.uint8, device="cuda")
        return cfg, ws

    def beam_admit(cfg, ws, enc_out):
        G = B // cfg.num_beams
        _libmod.check(lib.loco_decoder_pool_init(e._handle, B, T, S, p(ws), ws.numel(), st()))
        _libmod.check(lib.loco_decoder_pool_admit_beams(e._handle, B, T, S, C.byref(cfg), G, i32(range(G)), p(enc_out), T * 768, i32([T] * G), None,
                                                        i32([S] * G), p(ws), ws.numel(), st()))
        torch.cuda.synchronize()

    def beam_step(ws, i, parents=None):
        _libmod.check(lib.loco_decoder_pool_step_beam(e._handle, B, T, S, i, T, None, None, p(parents), p(ws), ws.numel(), st()))

    def beam_run(cfg, ws, enc_out, steps):
        beam_admit(cfg, ws, enc_out)
        return timed(lambda: [beam_step(ws, i) for i in range(steps)]) / steps

    # with synthetic weights a row ends at its first token or never: draw encoder rows until every slot outlives the longest run
    pools = {K: beam_pool(K) for K in (4, 16)}
    for seed in range(16):
        enc_out = torch.randn((B, T, 768), device="cuda", generator=torch.Generator("cuda").manual_seed(seed))
        greedy_run(enc_out, args.steps)
        ok = open_slots(gws) == B
        for K, (cfg, ws) in pools.items():
            beam_run(cfg, ws, enc_out, 405 if K == 4 else args.steps)
            ok = ok and open_slots(ws) == B
        if ok:
            break
    else:
        sys.exit("no draw of encoder rows keeps every slot open")
    # (i)
    runs = {"greedy_pool_step": [], "beam_step_K4": [], "beam_step_K16": []}
    for _ in range(9):
        runs["greedy_pool_step"].append(greedy_run(enc_out, args.steps))
        for K, (cfg, ws) in pools.items():
            runs[f"beam_step_K{K}"].append(beam_run(cfg, ws, enc_out, args.steps))
    res["step_ms"] = {k: dict(median=statistics.median(v), runs=v) for k, v in runs.items()}
    res["step_ms"]["steps_per_run"] = args.steps
    res["encoder_rows_seed"] = seed
    # (ii)
    cfg, ws = pools[4]
    beam_admit(cfg, ws, enc_out)
    parents = torch.zeros((405, B), dtype=torch.int32, device="cuda")
    per_step = [timed(lambda: beam_step(ws, i, parents[i])) for i in range(405)]
    assert open_slots(ws) == B
    moved = (parents.cpu() != torch.arange(B, dtype=torch.int32)[None, :]).sum(1).tolist()
    cache = torch.zeros((layers, B, S, 1536), dtype=torch.float32, device="cuda")
    shadow = torch.zeros_like(cache)
    rotate = torch.tensor([r // 4 * 4 + (r + 1) % 4 for r in range(B)], dtype=torch.int32, device="cuda")
    share = {}
    for pos in (10, 100, 400):
        count = torch.full((B,), pos + 1, dtype=torch.int32, device="cuda")
        once = lambda: _libmod.check(lib.loco_op_beam_reorder(p(cache), p(shadow), layers, B, S, 1536, p(rotate), p(count), None, 4, pos + 1, st()))  # noqa: E731
        once()
        alone = statistics.median(timed(once) for _ in range(9))
        step = statistics.median(per_step[pos - 4:pos + 5])
        share[str(pos)] = dict(step_ms=step, slots_that_changed_parent=moved[pos - 4:pos + 5], reorder_alone_every_slot_moves_ms=alone,
                               bytes_moved_every_slot=2 * layers * B * (pos + 1) * 1536 * 4, worst_case_share_of_step=alone / step)
    res["reorder_K4"] = share
    del cache, shadow
    # (iii)
    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    corpus_res = {}
    for name, fn in (("generate_many", lambda: model.generate_many(batches, max_length=caps, slots=64, pack=32)),
                     ("beam_search_many_K4", lambda: [per[0] for per in model.beam_search_many(batches, num_beams=4, max_length=caps, slots=64, pack=32)])):
        fn()  # warm-up
        s, rows = wall(fn)
        n = sum(len(r) - 1 for r in rows)
        corpus_res[name] = dict(seconds=s, tokens=n, tokens_per_s=n / s)
        print(name, corpus_res[name], flush=True)
    res["corpus"] = dict(utterances=args.utterances, caps="90 % in 10-60, 10 % at 450, Philox seed 5", **corpus_res)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
