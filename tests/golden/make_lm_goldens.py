"""Writes the language-model fixtures lm1.npz, lm2.npz and lm_windows.json.  CPU only.

    python tests/golden/make_lm_goldens.py [--reference DIR]

lm1 / lm2: HuggingFace's own GPT2LMHeadModel, loaded with synth.gpt2_state_dict (no weights are committed), run in fp32 and in float64 on
three equal-length rows (S = 17) and one ragged set (lengths 5, 17, 64; every sequence run unpadded, which causal attention makes
equivalent to right padding).  Stored: the ids, the float64 NLLs, probe rows of the float64 hidden states, and HF-fp32's OWN error against
float64 -- max abs NLL error and hidden-state relative L2 -- which is what the GPU tests' bars are multiples of.
  lm1: n_layer 2, n_positions 64, vocab 50257 (the real head size).   lm2: all 12 layers, vocab 1003.

lm_windows: the reference's two dataset classes (lms/src/utils.py, imported from --reference by this generator only, never by a test)
driven with a stub tokenizer at max_len = 8 on recordings of 3, 7, 8, 9 and 13 tokens plus a duplicate utterance id: the id lists
they yield and their first / last flags.
"""
import argparse
import importlib
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

LOGIT_SCALE = 3.0
EQUAL_S, RAGGED = 17, (5, 17, 64)


def hf_model(sd, n_layer, n_positions, vocab, dtype):
    import torch
    from transformers import GPT2Config, GPT2LMHeadModel
    m = GPT2LMHeadModel(GPT2Config(n_layer=n_layer, n_positions=n_positions, vocab_size=vocab, attn_pdrop=0.0, embd_pdrop=0.0, resid_pdrop=0.0))
    res = m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=False)
    assert not res.unexpected_keys and all(k.endswith((".attn.bias", ".attn.masked_bias")) for k in res.missing_keys), res
    return m.to(dtype).eval()


def run(model, ids):
    """(nll [B, S - 1], hidden states n_layer + 1 x [B, S, 768]) as float64 numpy."""
    import torch
    with torch.no_grad():
        out = model(torch.from_numpy(ids), output_hidden_states=True)
        logits = out.logits[:, :-1]
        nll = torch.nn.functional.cross_entropy(logits.transpose(1, 2), torch.from_numpy(ids)[:, 1:], reduction="none")
    return nll.double().numpy(), [h.double().numpy() for h in out.hidden_states]


def lm_fixture(name, n_layer, n_positions, vocab):
    import torch
    synth = importlib.import_module("loco-asr_amd.synth")
    sd = synth.gpt2_state_dict(0, n_layer, n_positions, vocab, LOGIT_SCALE)
    m32, m64 = hf_model(sd, n_layer, n_positions, vocab, torch.float32), hf_model(sd, n_layer, n_positions, vocab, torch.float64)
    seqs = [synth.gpt2_token_ids(EQUAL_S, vocab, f"{name}/eq{i}") for i in range(3)] + [synth.gpt2_token_ids(n, vocab, f"{name}/rag{i}")
                                                                                        for i, n in enumerate(RAGGED)]
    out = {"n_layer": n_layer, "n_positions": n_positions, "vocab": vocab, "logit_scale": LOGIT_SCALE, "seed": 0}
    nll_err, num, den = 0.0, np.zeros(n_layer + 1), np.zeros(n_layer + 1)
    logit_std = []
    groups = [np.stack(seqs[:3])] + [s[None] for s in seqs[3:]]  # the equal rows as ONE batch, the ragged ones alone
    k = 0
    for g in groups:
        n64, h64 = run(m64, g)
        n32, h32 = run(m32, g)
        nll_err = max(nll_err, float(np.abs(n32 - n64).max()))
        for b in range(len(g)):
            probes = np.asarray(sorted({0, len(g[b]) // 2, len(g[b]) - 1}) if k == 0 else [len(g[b]) - 1])
            out[f"ids{k}"] = g[b]
            out[f"nll{k}"] = n64[b]
            out[f"probe_pos{k}"] = probes
            out[f"probe{k}"] = np.stack([h[b][probes] for h in h64])  # [n_layer + 1, probes, 768] float64
            for i in range(n_layer + 1):
                num[i] += ((h32[i][b][probes] - h64[i][b][probes]) ** 2).sum()
                den[i] += (h64[i][b][probes] ** 2).sum()
            z = h64[-1][b] @ np.asarray(sd["transformer.wte.weight"], np.float64).T
            logit_std.append(float(z.std(-1).mean()))
            k += 1
    out["n_seq"] = k
    out["hf_fp32_nll_max_abs_err"] = nll_err
    out["hf_fp32_hidden_rel_l2"] = np.sqrt(num / den)  # per hidden state, over the probe rows
    out["logit_std"] = float(np.mean(logit_std))
    assert out["logit_std"] > 2.0, out["logit_std"]
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print(name, "nll err", nll_err, "hidden rel l2 max", out["hf_fp32_hidden_rel_l2"].max(), "logit std", out["logit_std"],
          "mean nll", float(np.mean([out[f"nll{i}"].mean() for i in range(k)])))


class StubTokenizer:
    bos_token_id, eos_token_id = 98, 99

    def __call__(self, text):
        return {"input_ids": [int(t) for t in text.split()]}


WINDOW_LINES = [  # (utt_id, text); out of time order on purpose, one utt_id twice
    ("rE-A-0200-0300", "40 41 42"),
    ("rA-A-0000-0100", "1 2"),
    ("rB-A-0100-0200", "13 14"),
    ("rB-B-0000-0100", "10 11 12"),
    ("rC-A-0000-0100", "20 21 22 23"),
    ("rC-B-0100-0200", "24 25"),
    ("rC-B-0100-0200", "77 77 77 77 77"),
    ("rD-B-0100-0200", "35 36"),
    ("rD-A-0000-0100", "30 31 32 33 34"),
    ("rE-B-0000-0100", "43 44 45 46"),
    ("rE-A-0300-0400", "47 48 49"),
]


def windows_fixture(reference):
    sys.path.insert(0, os.path.join(reference, "lms", "src"))
    import utils as ref_utils  # the read-only reference's dataset classes
    max_len, bsize = 8, 2
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "text")
        with open(path, "w") as fh:
            fh.writelines(f"{u} {t}\n" for u, t in WINDOW_LINES)
        indep = ref_utils.FisherTextDatasetIndep(path, StubTokenizer(), batch_size=bsize)
        indep_out = {"utt_ids": list(indep.utt_ids), "batches": [[list(map(int, s)) for s in b] for b in indep]}
        ml = ref_utils.FisherTextDatasetMaxLen(path, StubTokenizer(), max_len=max_len, batch_size=bsize)
        ml_out = [{"batch": [list(map(int, s)) for s in b], "rec_ids": list(r), "first": bool(f), "last": bool(l)} for b, r, f, l in ml]
        lens = {k: len(v) for k, v in ml.rec_id2text.items()}
    assert sorted(lens.values()) == [3, 7, 8, 9, 13], lens
    with open(os.path.join(HERE, "lm_windows.json"), "w") as fh:
        json.dump({"lines": WINDOW_LINES, "max_len": max_len, "bsize": bsize, "bos": 98, "eos": 99, "recording_tokens": lens, "indep": indep_out,
                   "max_len_batches": ml_out}, fh, indent=1)
    print("lm_windows", lens, len(ml_out), "max_len batches")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=None, help="checkout of the reference project (for lm_windows.json only)")
    a = ap.parse_args()
    lm_fixture("lm1", 2, 64, 50257)
    lm_fixture("lm2", 12, 64, 1003)
    if a.reference:
        windows_fixture(a.reference)
