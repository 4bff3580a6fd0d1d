"""Writes the cached-context fixture lm3.npz.  CPU only.

    python tests/golden/make_lm_context_goldens.py

lm3: HuggingFace's own GPT2LMHeadModel, loaded with synth.gpt2_state_dict (no weights are committed) at n_layer 2, n_positions 320, vocab
1003, logit_scale 3, seed 0 -- long enough for a cached prefix of several key tiles -- run in fp32 and in float64 on three sequences of
320, 130 and 66 tokens.  Stored: the ids, the float64 NLL of every position but the first, and HF-fp32's OWN largest NLL error against
float64, which the GPU tests' bar is a multiple of.

The generator also checks that scoring behind a cached context is the same quantity as scoring in one pass: HF's own past_key_values
evaluation in float64 (prefix first, the rest behind its cache) must equal the uncached evaluation at several cuts.
"""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_lm_goldens import hf_model  # noqa: E402

N_LAYER, N_POSITIONS, VOCAB, LOGIT_SCALE, SEED = 2, 320, 1003, 3.0, 0
LENGTHS = (320, 130, 66)
CUTS = (1, 63, 64, 65, 257)


def nll_of(logits, targets):
    import torch
    return torch.nn.functional.cross_entropy(logits, targets, reduction="none")


def uncached(model, ids):
    import torch
    t = torch.from_numpy(ids)[None]
    with torch.no_grad():
        return nll_of(model(t).logits[0, :-1], t[0, 1:]).double().numpy()


def cached(model, ids, cut):
    """The NLLs of ids[cut:] behind HF's own cache of ids[:cut]."""
    import torch
    t = torch.from_numpy(ids)[None]
    with torch.no_grad():
        pre = model(t[:, :cut], use_cache=True)
        rest = model(t[:, cut:], past_key_values=pre.past_key_values, use_cache=True)
        logits = torch.cat([pre.logits[0, -1:], rest.logits[0, :-1]])
        return nll_of(logits, t[0, cut:]).double().numpy()


def main():
    import torch
    synth = importlib.import_module("loco-asr_amd.synth")
    sd = synth.gpt2_state_dict(SEED, N_LAYER, N_POSITIONS, VOCAB, LOGIT_SCALE)
    m32, m64 = (hf_model(sd, N_LAYER, N_POSITIONS, VOCAB, dt) for dt in (torch.float32, torch.float64))
    out = {"n_layer": N_LAYER, "n_positions": N_POSITIONS, "vocab": VOCAB, "logit_scale": LOGIT_SCALE, "seed": SEED, "n_seq": len(LENGTHS)}
    err = cache_gap = 0.0
    for k, n in enumerate(LENGTHS):
        ids = synth.gpt2_token_ids(n, VOCAB, f"lm3/seq{k}")
        n64 = uncached(m64, ids)
        err = max(err, float(np.abs(uncached(m32, ids) - n64).max()))
        for cut in CUTS:
            if cut < n:
                cache_gap = max(cache_gap, float(np.abs(cached(m64, ids, cut) - n64[cut - 1:]).max()))
        out[f"ids{k}"] = ids
        out[f"nll{k}"] = n64
    assert cache_gap < 1e-12, cache_gap  # cached and uncached scoring are the same quantity
    out["hf_fp32_nll_max_abs_err"] = err
    out["hf_f64_cached_vs_uncached_max_abs"] = cache_gap
    np.savez_compressed(os.path.join(HERE, "lm3.npz"), **out)
    print("lm3 nll err", err, "cached vs uncached (float64)", cache_gap, "mean nll", float(np.mean([out[f"nll{k}"].mean() for k in range(len(LENGTHS))])))


if __name__ == "__main__":
    main()
