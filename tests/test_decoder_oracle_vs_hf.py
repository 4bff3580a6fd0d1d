"""Direct comparison of the decoder oracle with the installed HuggingFace modules (skipped where transformers is absent).
Complements fixture g13: another decoder seed, other shapes, frame counts of 1 / 63 / 64 / 65, <pad> inside and at the end of rows,
and HF's cached step (past_key_values) against the oracle's greedy loop."""
import numpy as np
import pytest
import torch

import speecht5_decoder_oracle as dec_oracle
from conftest import rel_l2

tr = pytest.importorskip("transformers")

SEED = 5


@pytest.fixture(scope="module")
def hf_and_sd(synth):
    sd = synth.decoder_state_dict(SEED)
    model = tr.SpeechT5ForSpeechToText(tr.SpeechT5Config()).eval()
    hf_sd = {(k if k.startswith("text_decoder_postnet.") else "speecht5." + k): torch.from_numpy(v) for k, v in sd.items()}
    missing, unexpected = model.load_state_dict(hf_sd, strict=False)
    assert not unexpected and not any(".decoder." in k and "embed_positions" not in k for k in missing), (missing, unexpected)
    return model.double(), sd


def inputs(synth, B, S, T, frames, tag):
    enc = synth.hashed_uniform(f"dec_vs_hf/{tag}", (B, T, 768), SEED).astype(np.float32)
    ids, _ = synth.token_ids(B, S, seed=SEED)
    ids[:, 0] = 2
    if S > 4:
        ids[0, 2] = 1        # <pad> inside a row
        ids[-1, 3:] = 1      # a row that is all <pad> after position 3
        ids[0, 4], ids[0, S - 1] = 0, 80
    mask = (np.arange(T)[None, :] < np.asarray(frames)[:, None]).astype(np.int64)
    return enc, ids, mask


@pytest.mark.parametrize("B,S,T,frames", [(1, 1, 1, [1]), (4, 9, 70, [65, 64, 63, 1]), (2, 33, 20, [20, 7])])
def test_forward_matches_hf(hf_and_sd, synth, B, S, T, frames):
    model, sd = hf_and_sd
    enc, ids, mask = inputs(synth, B, S, T, frames, f"{B}/{S}/{T}")
    with torch.no_grad():
        r = model.speecht5.decoder(input_values=torch.from_numpy(ids), encoder_hidden_states=torch.from_numpy(enc).double(),
                                   encoder_attention_mask=torch.from_numpy(mask), output_hidden_states=True)
        want = model.text_decoder_postnet(r.last_hidden_state)
    hs = []
    got = dec_oracle.forward(enc, frames, ids, sd, torch.float64, hs)
    assert rel_l2(got, want) <= 1e-9, rel_l2(got, want)
    assert len(hs) == len(r.hidden_states) == 7
    for h, w in zip(hs, r.hidden_states):
        assert rel_l2(h, w) <= 1e-9
    # frames None = HF without an encoder mask
    with torch.no_grad():
        r = model.speecht5.decoder(input_values=torch.from_numpy(ids), encoder_hidden_states=torch.from_numpy(enc).double())
        want = model.text_decoder_postnet(r.last_hidden_state)
    assert rel_l2(dec_oracle.forward(enc, None, ids, sd), want) <= 1e-9


def test_greedy_steps_match_hf_cached_path(hf_and_sd, synth):
    """HF's one-token-per-call path along the oracle's own ids: every step's logits, finished (<pad>-fed) rows included."""
    model, sd = hf_and_sd
    frames = [40, 17, 1]
    enc, _, mask = inputs(synth, 3, 1, 40, frames, "greedy")
    ids, steps, lengths, gaps = dec_oracle.greedy(enc, frames, sd, 12)
    assert ids.shape[1] <= 12 and bool((ids[:, 0] == 2).all())
    past, want = None, []
    with torch.no_grad():
        for t in range(ids.shape[1] - 1):
            r = model.speecht5.decoder(input_values=ids[:, t:t + 1], encoder_hidden_states=torch.from_numpy(enc).double(),
                                       encoder_attention_mask=torch.from_numpy(mask), past_key_values=past, use_cache=True)
            past = r.past_key_values
            want.append(model.text_decoder_postnet(r.last_hidden_state)[:, 0])
    want = torch.stack(want)
    assert rel_l2(steps, want) <= 1e-9, rel_l2(steps, want)
    for b in range(3):  # the layout HF's generate leaves: argmax until </s>, <pad> after it
        done = False
        for t in range(ids.shape[1] - 1):
            assert int(ids[b, t + 1]) == (1 if done else int(want[t, b].argmax())), (b, t)
            done = done or int(ids[b, t + 1]) == 2
        assert int(lengths[b]) == (int((ids[b, 1:] == 2).nonzero()[0]) + 2 if bool((ids[b, 1:] == 2).any()) else ids.shape[1])
