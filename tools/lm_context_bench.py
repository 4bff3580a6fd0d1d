#!/usr/bin/env python3
"""What the GPT-2 scorer's cached context costs on one MI355X (no ratio is fixed in advance: nobody had run this kernel).

  (a) `carry` mode on one recording of --recording-tokens tokens at n_positions 1024, keep 512, through lm.score_carry; beside it the
      `max_len` figure of the same recording length, read from --max-len-json (tools/lm_bench.py's output, re-measured on the same box);
  (b) lm.rescore with a context of P = 900 tokens and N = 16 hypotheses of L = 24; beside it the way without a cache: token_nll on the 16
      concatenated sequences of 924 tokens;
  (c) the attention kernel alone (loco_op_lm_ctx_attention) against loco_op_decoder_attention on the shape of (b);
  (d) one loco_lm_nll batch of 128 x 100 tokens: the path that existed before, to show it is where it was.

Host clock around synchronised work, as tools/lm_bench.py.  Synthetic 12-layer weights, V = 50 257.  Writes one JSON object (default
profiles/lm_context_cost.json).
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
    ap.add_argument("--recording-tokens", type=int, default=3000)
    ap.add_argument("--keep", type=int, default=512)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--max-len-json", default=None, help="tools/lm_bench.py's output measured on the same box: its max_len block is copied beside (a)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lm_context_cost.json"))
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
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    # ---- (d) the path that was there: one batch of 128 x 100 ----
    B, S = 128, 100
    ids = torch.from_numpy(la.synth.gpt2_token_ids(B * S, V, "bench/batch").astype(np.int32)).cuda()
    rows = (np.arange(B)[:, None] * S + np.arange(S - 1)[None, :]).reshape(-1)
    batch_s, _ = timed(lambda: model.nll_rows(ids, np.arange(B) * S, [S] * B, S, rows), 5)
    res["parent_path_batch_128x100"] = {"batch_ms": batch_s * 1e3, "tokens_per_s": B * S / batch_s}
    print(json.dumps(res["parent_path_batch_128x100"]), flush=True)
    save()

    # ---- (a) carry mode over one recording cut into utterances ----
    n, lens, cycle = a.recording_tokens, [], [4, 8, 12, 20, 30, 50, 80]
    while sum(lens) < n:
        lens.append(min(cycle[len(lens) % len(cycle)] + 1, n - sum(lens)))
    utts = {f"rec000-A-{i:06d}-{i:06d}": " ".join(map(str, la.synth.gpt2_token_ids(m - 1, V - 1, f"bench/c{i}"))) if m > 1 else "" for i, m in enumerate(lens)}
    plan = list(lm.carry_plan(lens, 1024, a.keep))
    carry_s, (nlls, _) = timed(lambda: lm.score_carry(model, utts, tok, keep=a.keep, inflight=1), 2)
    res["carry"] = {"recording_tokens": n, "utterances": len(lens), "keep": a.keep, "chunks": len(plan), "rebases": sum(c[4] for c in plan),
                    "prefilled_tokens": sum(c[1] for c in plan if c[4]), "scored": len(nlls["rec000"]), "seconds": carry_s,
                    "scored_tokens_per_s": len(nlls["rec000"]) / carry_s}
    if a.max_len_json:
        with open(a.max_len_json) as fh:
            res["max_len_same_box"] = json.load(fh)["max_len"]
        res["carry"]["speedup_over_max_len_scored_tokens_per_s"] = res["carry"]["scored_tokens_per_s"] / res["max_len_same_box"]["scored_tokens_per_s"]
    print(json.dumps(res["carry"]), flush=True)
    save()

    # ---- (b) rescore: 16 hypotheses of 24 tokens behind 900 tokens of context ----
    P, N, L = 900, 16, 24
    ctx = torch.from_numpy(la.synth.gpt2_token_ids(P, V, "bench/ctx")).cuda()
    hyps = [torch.from_numpy(la.synth.gpt2_token_ids(L, V, f"bench/h{i}")).cuda() for i in range(N)]
    cached_s, (got, _) = timed(lambda: lm.rescore(model, ctx, hyps), 5)
    cat = torch.stack([torch.cat([ctx, h]) for h in hyps])
    concat_s, full = timed(lambda: model.token_nll(cat), 3)
    cache = model.new_cache(1)
    model.append(cache, 0, ctx)
    score_s, _ = timed(lambda: model.token_nll_given(cache, hyps, slots=0), 5)
    gap = max(float((g.double() - f[P - 1:].double()).abs().max()) for g, f in zip(got, full))
    res["rescore"] = {"P": P, "N": N, "L": L, "rescore_ms": cached_s * 1e3, "of_which_scoring_ms": score_s * 1e3, "concatenated_token_nll_ms": concat_s * 1e3,
                      "speedup": concat_s / cached_s, "max_abs_nll_difference": gap}
    print(json.dumps(res["rescore"]), flush=True)
    save()
    del cache

    # ---- (c) the kernel alone on that shape, against the wave-per-row attention ----
    rows_n = N * L
    qkv = torch.randn(rows_n, 2304, device="cuda")
    kc, vc = torch.randn(1, 1024, 768, device="cuda"), torch.randn(1, 1024, 768, device="cuda")
    out = torch.empty(rows_n, 768, device="cuda")
    seqs = (C.c_int32 * (3 * N))(*[x for _ in range(N) for x in (L, 0, P)])
    new_s, _ = timed(lambda: _lib.check(lib.loco_op_lm_ctx_attention(p(qkv), p(kc), p(vc), 1024 * 768, seqs, N, 1, p(out), st)), 20)
    q = qkv.view(N, L, 2304)[:, :, :768].contiguous()
    k = torch.cat([kc[:, :P].expand(N, -1, -1), qkv.view(N, L, 2304)[:, :, 768:1536]], 1).contiguous()
    v = torch.cat([vc[:, :P].expand(N, -1, -1), qkv.view(N, L, 2304)[:, :, 1536:]], 1).contiguous()
    nb = int(lib.loco_decoder_attention_scratch_bytes(N, L, P + L))
    scratch, out2 = torch.empty(max(nb, 4), dtype=torch.uint8, device="cuda"), torch.empty(N, L, 768, device="cuda")
    old_s, _ = timed(lambda: _lib.check(lib.loco_op_decoder_attention(p(q), p(k), p(v), None, p(out2), N, L, P + L, 1, P, 0.125, p(scratch), scratch.numel(), st)),
                     20)
    res["kernel_alone"] = {"N": N, "L": L, "P": P, "lm_ctx_attention_us": new_s * 1e6, "decoder_attention_us": old_s * 1e6, "speedup": old_s / new_s,
                           "rel_l2_between_them": float((out.view(N, L, 768) - out2).norm() / out2.norm()),
                           "kv_bytes_read_per_layer_wave_per_row": 2 * 4 * 64 * 12 * rows_n * (P + L), "kv_bytes_read_per_layer_tiled": 2 * 4 * 64 * 12 * N * (P + L)}
    print(json.dumps(res["kernel_alone"]), flush=True)
    save()


if __name__ == "__main__":
    main()
