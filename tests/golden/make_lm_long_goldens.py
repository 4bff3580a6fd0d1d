"""Writes the long-sequence fixture lm4.npz: the scorer at GPT-2's own lengths.  CPU only.

    python tests/golden/make_lm_long_goldens.py

lm4: HuggingFace's own GPT2LMHeadModel, loaded with synth.gpt2_state_dict (no weights are committed) at n_layer 2, n_positions 1024, vocab
1003, logit_scale 3, seed 0, run in fp32 and in float64 on six sequences of 1024, 700, 341, 300, 257 and 130 tokens and on one "recording"
of 1030 tokens walked at max_len = 1024.  Stored:

  ids{k}, nll{k}      the ids and the float64 NLL of every position but the first;
  rec_ids, rec_nll    the recording and the rows the reference's max_len walk scores (tests/lm_ref.max_len_batches): window 0's NLLs in
                      full, then the last position's NLL of windows 1 .. 5 -- targets 1 .. 1028, never the final token;
  probe_pos, probe    sequence 0's float64 hidden states (all n_layer + 1) at rows on both sides of the 64-, 256- and 512-row boundaries;
  hf_fp32_nll_max_abs_err, hf_fp32_hidden_rel_l2
                      HF-fp32's OWN error against float64 over everything stored, which the GPU tests' bars are multiples of;
  hf_f64_cached_vs_uncached_max_abs, logit_std.

The NLLs are stored as float64; the probes too (8 rows x 3 states x 768), which keeps the file near 70 KB.

The generator checks that scoring behind a cached context is the same quantity as scoring in one pass -- HF's own past_key_values
evaluation in float64 equals the uncached one at every cut the GPU tests use, within 1e-12 -- so one set of NLLs serves both paths, and
that the softmax is far from flat (logit_std > 2).  tests/test_lm_long_ref.py checks on the CPU that planted attention faults move these
NLLs by at least 10 x the GPU bar; with logit_scale 3 and synth's c_attn scale they do (no extra scaling was needed here).  If that test
ever fails, raise LOGIT_SCALE or scale c_attn HERE until it passes, and say so in this docstring.
"""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_lm_context_goldens import cached  # noqa: E402
from make_lm_goldens import hf_model, run  # noqa: E402

N_LAYER, N_POSITIONS, VOCAB, LOGIT_SCALE, SEED = 2, 1024, 1003, 3.0, 0
LENGTHS = (1024, 700, 341, 300, 257, 130)
REC_TOKENS, MAX_LEN = 1030, 1024
CUTS = (511, 512, 513, 895, 1023)
PROBE_ROWS = (0, 63, 64, 255, 256, 511, 512, 1023)


def main():
    import torch
    synth = importlib.import_module("loco-asr_amd.synth")
    sd = synth.gpt2_state_dict(SEED, N_LAYER, N_POSITIONS, VOCAB, LOGIT_SCALE)
    m32, m64 = (hf_model(sd, N_LAYER, N_POSITIONS, VOCAB, dt) for dt in (torch.float32, torch.float64))
    out = {"n_layer": N_LAYER, "n_positions": N_POSITIONS, "vocab": VOCAB, "logit_scale": LOGIT_SCALE, "seed": SEED, "n_seq": len(LENGTHS),
           "max_len": MAX_LEN}
    err = cache_gap = 0.0
    logit_std = []
    wte = np.asarray(sd["transformer.wte.weight"], np.float64)
    for k, n in enumerate(LENGTHS):
        ids = synth.gpt2_token_ids(n, VOCAB, f"lm4/seq{k}")
        n64, h64 = run(m64, ids[None])
        n32, h32 = run(m32, ids[None])
        err = max(err, float(np.abs(n32 - n64).max()))
        out[f"ids{k}"] = ids
        out[f"nll{k}"] = n64[0]
        logit_std.append(float((h64[-1][0] @ wte.T).std(-1).mean()))
        if k == 0:
            pos = np.asarray(PROBE_ROWS)
            out["probe_pos"] = pos
            out["probe"] = np.stack([h[0][pos] for h in h64])  # [n_layer + 1, probes, 768] float64
            num = np.asarray([((a[0][pos] - b[0][pos]) ** 2).sum() for a, b in zip(h32, h64)])
            den = np.asarray([(b[0][pos] ** 2).sum() for b in h64])
            out["hf_fp32_hidden_rel_l2"] = np.sqrt(num / den)  # per hidden state, over the probe rows
            for cut in CUTS:
                cache_gap = max(cache_gap, float(np.abs(cached(m64, ids, cut) - n64[0][cut - 1:]).max()))
    assert cache_gap < 1e-12, cache_gap  # cached and uncached scoring are the same quantity

    rec = synth.gpt2_token_ids(REC_TOKENS, VOCAB, "lm4/rec")
    wins = np.stack([rec[o:o + MAX_LEN] for o in range(REC_TOKENS - MAX_LEN)])  # never the window that ends at the final token
    w64, w32 = run(m64, wins)[0], run(m32, wins)[0]
    pick = lambda w: np.concatenate([w[0], w[1:, -1]])  # noqa: E731
    err = max(err, float(np.abs(pick(w32) - pick(w64)).max()))
    out["rec_ids"] = rec
    out["rec_nll"] = pick(w64)
    assert len(out["rec_nll"]) == REC_TOKENS - 2

    out["hf_fp32_nll_max_abs_err"] = err
    out["hf_f64_cached_vs_uncached_max_abs"] = cache_gap
    out["logit_std"] = float(np.mean(logit_std))
    assert out["logit_std"] > 2.0, out["logit_std"]
    path = os.path.join(HERE, "lm4.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 400_000, os.path.getsize(path)
    print("lm4 nll err", err, "hidden rel l2", out["hf_fp32_hidden_rel_l2"].tolist(), "cached vs uncached (float64)", cache_gap,
          "logit std", out["logit_std"], "mean nll", float(np.mean([out[f"nll{k}"].mean() for k in range(len(LENGTHS))])),
          "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
