#!/usr/bin/env python3
"""Generate tests/golden/g12_attentions.npz: HF's attention probabilities (output_attentions=True) for the speech and text
encoders, computed in float64 from the deterministic weights of ``loco-asr_amd/synth.py``.

Run in the build container only (it imports ``transformers``):

    python tests/golden/make_attention_goldens.py

Contents (fp32, rounded to multiples of 2^-24 so that the file compresses below 1 MiB: |error| <= 3e-8 against HF's float64;
masked keys are exactly 0, in HF as here):
  g1_probs        [3, 1, 12, 49, 49]   full P of layers G1_LAYERS for g1's 1 s clip (T = 49)
  g2_long_rows    [12, 12, 3, 249]     layers x heads x G2_LONG_ROWS x keys, the 5 s clip of g2's ragged 5 s + 3 s pair
  g2_short_rows   [12, 12, 5, 249]     the same for its 3 s clip, rows G2_SHORT_ROWS
  text_rows       [3, 3, 12, 5, 57]    layers TEXT_LAYERS x clips x heads x TEXT_ROWS x keys for g6's masked token ids
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens as mg  # noqa: E402  (hf_encoder, synth)

synth = mg.synth
G1_LENGTHS = [16000]
G1_LAYERS = [0, 6, 11]
G2_LENGTHS = [80000, 48000]
G2_LONG_ROWS = [0, 1, 248]               # first two, T - 1 (all valid)
G2_SHORT_ROWS = [0, 1, 148, 149, 248]     # first two, the 3 s clip's last valid frame, its first padded frame, T - 1
GRID = 2.0 ** -24
TEXT_LENGTHS = [57, 31, 44]
TEXT_LAYERS = [0, 6, 11]
TEXT_ROWS = [0, 1, 30, 31, 56]  # the 31-token clip's last valid token and first pad token, T - 1


def _speech_attn(enc, lengths):
    x, m = synth.batch(lengths)
    with torch.no_grad():
        res = enc(input_values=torch.from_numpy(x).double(), attention_mask=torch.from_numpy(m), output_attentions=True)
    return [a.numpy() for a in res.attentions]


def text_encoder(enc):
    from transformers import SpeechT5Config
    from transformers.models.speecht5.modeling_speecht5 import SpeechT5EncoderWithTextPrenet

    tenc = SpeechT5EncoderWithTextPrenet(SpeechT5Config()).eval()
    assert tenc.config._attn_implementation == "eager"
    tsd = synth.text_prenet_state_dict(0)
    sd = {"prenet." + k[len("text_prenet."):]: torch.from_numpy(np.asarray(v)) for k, v in tsd.items()}
    sd.update({k: v for k, v in enc.state_dict().items() if k.startswith("wrapped_encoder.")})
    tenc.load_state_dict(sd, strict=True)
    return tenc


def _q(a):
    return (np.round(np.asarray(a, np.float64) / GRID) * GRID).astype(np.float32)


def compute():
    """-> dict of the fixture's arrays, from HF in float64."""
    sd = synth.encoder_state_dict(0)
    enc = mg.hf_encoder(sd)
    tenc = text_encoder(enc).double()
    enc = enc.double()
    g1 = _speech_attn(enc, G1_LENGTHS)
    g2 = _speech_attn(enc, G2_LENGTHS)
    ids, mask = synth.token_ids(3, 57, lengths=TEXT_LENGTHS)
    with torch.no_grad():
        t = tenc(torch.from_numpy(ids), attention_mask=torch.from_numpy(mask), output_attentions=True).attentions
    return dict(g1_lengths=np.array(G1_LENGTHS), g1_layers=np.array(G1_LAYERS),
                g1_probs=_q(np.stack([g1[l] for l in G1_LAYERS])),
                g2_lengths=np.array(G2_LENGTHS), g2_long_rows_index=np.array(G2_LONG_ROWS), g2_short_rows_index=np.array(G2_SHORT_ROWS),
                g2_long_rows=_q(np.stack([a[0][:, G2_LONG_ROWS] for a in g2])),
                g2_short_rows=_q(np.stack([a[1][:, G2_SHORT_ROWS] for a in g2])),
                text_lengths=np.array(TEXT_LENGTHS), text_layers=np.array(TEXT_LAYERS), text_rows_index=np.array(TEXT_ROWS),
                text_rows=_q(np.stack([t[l].numpy()[:, :, TEXT_ROWS] for l in TEXT_LAYERS])))


def main():
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    arrs = compute()
    path = os.path.join(HERE, "g12_attentions.npz")
    np.savez_compressed(path, **arrs)
    print(f"wrote g12_attentions.npz: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
