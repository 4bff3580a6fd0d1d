#!/usr/bin/env python3
"""What the GPT-2 scorer costs on one MI355X (no bar: nobody has run this before).

  * `indep` mode at bsize 128 over a synthetic length-binned corpus (utterance lengths as a conversational corpus has them: many short,
    few long), tokens/s end to end through lm.score_indep (ids uploaded once, fold included);
  * one recording of --recording-tokens tokens through `max_len` mode at n_positions 1024 (every window re-runs the body: absolute
    positions restart, nothing is reusable), tokens scored per second and body tokens per second;
  * the LM head alone on the rows of one 128 x 100 batch: its share of that batch's time and its fraction of the 157.3 TFLOP/s fp32 MFMA peak.

Writes one JSON object (default profiles/lm_cost.json).  Synthetic weights (synth.gpt2_state_dict): the arithmetic does not depend on them.
"""
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
_lib = importlib.import_module("loco-asr_amd._lib")
lm = la.lm
PEAK_FP32_MFMA = 157.3e12
V = 50257


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps, out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--utterances", type=int, default=4096)
    ap.add_argument("--recording-tokens", type=int, default=3000)
    ap.add_argument("--bsize", type=int, default=128)
    ap.add_argument("--max-len-bsize", type=int, default=32)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lm_cost.json"))
    a = ap.parse_args()
    lib = _lib.load()
    res = {"device": torch.cuda.get_device_name(0), "layers": a.layers, "vocab": V, "n_positions": 1024}

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)

    sd = la.synth.gpt2_state_dict(0, a.layers, 1024, V)
    model = la.GPT2LMHeadModelMI355X.from_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}).to("cuda")
    del sd
    tok = lm.TokenizedLines(eos_token_id=V - 1)

    # ---- the head alone, and its share of one batch of 128 x 100 ----
    B, S = 128, 100
    ids = torch.from_numpy(la.synth.gpt2_token_ids(B * S, V, "bench/batch").astype(np.int32)).cuda()
    rows = (np.arange(B)[:, None] * S + np.arange(S - 1)[None, :]).reshape(-1)
    batch_s, _ = timed(lambda: model.nll_rows(ids, np.arange(B) * S, [S] * B, S, rows), 5)
    R = len(rows)
    h = torch.randn(R, 768, device="cuda")
    w = torch.randn(V, 768, device="cuda") * 0.1
    t = torch.randint(0, V, (R,), dtype=torch.int32, device="cuda")
    nb = int(lib.loco_lm_head_scratch_bytes(R, V))
    scratch, out = torch.empty(nb, dtype=torch.uint8, device="cuda"), torch.empty(R, device="cuda")
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    head_s, _ = timed(lambda: _lib.check(lib.loco_op_lm_head_nll(p(h), 768, p(w), 768, p(t), R, V, -100, p(out), p(scratch), nb, st)), 10)
    flops = 2.0 * R * V * 768
    res["batch_128x100"] = {"rows_scored": R, "batch_ms": batch_s * 1e3, "head_ms": head_s * 1e3, "head_share_of_time": head_s / batch_s,
                            "head_tflops": flops / head_s / 1e12, "head_fraction_of_fp32_mfma_peak": flops / head_s / PEAK_FP32_MFMA,
                            "logits_bytes_not_written": R * V * 4, "tokens_per_s": B * S / batch_s}
    print(json.dumps(res["batch_128x100"]), flush=True)
    save()

    # ---- indep mode over a length-binned corpus ----
    rng = np.random.default_rng(0)
    lens = rng.choice([4, 8, 12, 20, 30, 50, 80], size=a.utterances, p=[0.2, 0.25, 0.2, 0.15, 0.1, 0.07, 0.03])
    utts = {f"rec{i % 40:03d}-A-{i:06d}-{i:06d}": " ".join(map(str, la.synth.gpt2_token_ids(int(n), V - 1, f"bench/u{i}"))) for i, n in enumerate(lens)}
    n_tok = int(lens.sum() + 2 * len(lens))
    indep_s, (nlls, ppl) = timed(lambda: lm.score_indep(model, utts, tok, a.bsize), 2)
    res["indep"] = {"utterances": a.utterances, "tokens": n_tok, "scored": sum(len(v) for v in nlls.values()), "bsize": a.bsize, "seconds": indep_s,
                    "tokens_per_s": n_tok / indep_s, "recordings": len(ppl)}
    print(json.dumps(res["indep"]), flush=True)
    save()

    # ---- max_len mode over one recording ----
    n = a.recording_tokens
    rec = {"rec000-A-000000-000001": " ".join(map(str, la.synth.gpt2_token_ids(n - 1, V - 1, "bench/recording")))}
    t0 = time.perf_counter()
    nlls, ppl = lm.score_max_len(model, rec, tok, a.max_len_bsize)
    torch.cuda.synchronize()
    ml_s = time.perf_counter() - t0
    windows = max(n - 1024, 1)
    res["max_len"] = {"recording_tokens": n, "windows": windows, "bsize": a.max_len_bsize, "scored": len(nlls["rec000"]), "seconds": ml_s,
                      "scored_tokens_per_s": len(nlls["rec000"]) / ml_s, "body_tokens_per_s": windows * 1024 / ml_s}
    print(json.dumps(res["max_len"]), flush=True)
    save()


if __name__ == "__main__":
    main()
