#!/usr/bin/env python3
"""Decode-step timings -> profiles/decoder_generate.json (tools, not bench.py): ms per step and tokens/s at B x T_enc, the step against
its byte floor, loco_decoder_begin (cross k|v projection) next to the encoder's forward, and the reference's operating point
(encoder + generate(max_length=100) for a pair of 5 s clips).  Warm-up first, medians of --reps runs, timed with events on the stream."""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
la = importlib.import_module("loco-asr_amd")
_libmod = importlib.import_module("loco-asr_amd._lib")

STREAM_RATE = 5.9e12  # bytes/s: layernorm_kernel's measured streaming rate
LAUNCHES_PER_STEP = 1 + 6 * 11 + 2  # + 1 combine per attention whose key range is split
GAP_US = 1.5  # per dependent kernel boundary (1.2-1.9 us measured on this part)


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
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decoder_generate.json"))
    ap.add_argument("--skip-long", action="store_true")
    args = ap.parse_args()
    t = lambda d: {k: torch.from_numpy(v) for k, v in d.items()}  # noqa: E731
    pre, enc = la.synth.split_state_dict(la.synth.encoder_state_dict(0))
    dec, post = la.synth.split_decoder_state_dict(la.synth.decoder_state_dict(0))
    model = la.SpeechT5ForSpeechToTextMI355X.from_state_dicts(t(pre), t(enc), decoder_state_dict=t(dec), postnet_state_dict=t(post)).to("cuda")
    lib, e = _libmod.load(), model.speecht5.encoder
    x, m = la.synth.batch([80000, 80000])
    xd, md = torch.from_numpy(x).cuda(), torch.from_numpy(m).cuda()
    model.generate(xd, md, max_length=8)  # loads the weights
    res = {"clock_state": "as found (not pinned)", "reps": args.reps, "steps_timed": args.steps, "grid": []}
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    S = args.steps + 1
    weight_bytes = 4.0 * (6 * (4 * 768 * 768 + 768 * 768 + 768 * 768 + 2 * 768 * 3072) + 81 * 768)
    for B in (1, 2, 32):
        for T in ((249, 1499) if args.skip_long else (249, 1499, 29999)):
            if B == 32 and T == 29999:
                continue  # 32 ten-minute clips: 35 GB of cross k|v, not a shape anyone decodes
            enc_out = torch.randn((B, T, 768), device="cuda")
            need = int(lib.loco_decoder_workspace_bytes(e._handle, B, T, S))
            ws = torch.empty(need, dtype=torch.uint8, device="cuda")
            p = lambda tn: C.c_void_p(tn.data_ptr())  # noqa: E731
            begin = lambda: _libmod.check(lib.loco_decoder_begin(e._handle, p(enc_out), None, B, T, S, p(ws), need, st()))  # noqa: E731

            def steps():
                for i in range(args.steps):
                    _libmod.check(lib.loco_decoder_step(e._handle, B, T, S, i, None, p(ws), need, st()))
            begin()
            ms_begin = timed(begin, args.reps)
            ms = timed(steps, args.reps) / args.steps
            kv = 4.0 * 6 * B * (2 * 768 * T + 2 * 768 * (args.steps / 2))
            floor_ms = (weight_bytes + kv) / STREAM_RATE * 1e3
            res["grid"].append(dict(B=B, T_enc=T, ms_per_step=ms, tokens_per_s=B / ms * 1e3, begin_ms=ms_begin, byte_floor_ms=floor_ms,
                                    ratio_to_floor=ms / floor_ms, launches_per_step=LAUNCHES_PER_STEP,
                                    gap_share_estimate=LAUNCHES_PER_STEP * GAP_US * 1e-3 / ms))
            print(res["grid"][-1], flush=True)
            del ws, enc_out
    enc_ms = timed(lambda: e(input_values=xd, attention_mask=md), args.reps)
    total = timed(lambda: model.generate(xd, md, max_length=100), args.reps)
    res["reference_point_2x5s"] = dict(encoder_ms=enc_ms, encoder_plus_generate100_ms=total)
    for name, (B, sec) in {"begin_30s_x32": (32, 30), "begin_10min_x4": (4, 600)}.items():
        if args.skip_long and sec == 600:
            res[name] = "not measured"
            continue
        T = int(lib.loco_output_frames(sec * 16000))
        enc_out = torch.randn((B, T, 768), device="cuda")
        need = int(lib.loco_decoder_workspace_bytes(e._handle, B, T, 8))
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        xe = torch.randn((B, sec * 16000), device="cuda") * 0.1
        enc_step_ms = timed(lambda: e(input_values=xe), max(2, args.reps // 2), warmup=1)  # the encoder's forward at the same shape, same run
        del xe
        res[name] = dict(T_enc=T, begin_ms=timed(lambda: _libmod.check(lib.loco_decoder_begin(e._handle, C.c_void_p(enc_out.data_ptr()), None, B, T, 8,
                                                                                             C.c_void_p(ws.data_ptr()), need, st())), args.reps),
                         mode="f32", encoder_step_ms=enc_step_ms)
        res[name]["begin_share_of_encoder"] = res[name]["begin_ms"] / enc_step_ms
        del ws, enc_out
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
