"""Pins the decoder oracle (oracle/speecht5_decoder_oracle.py) to HuggingFace through fixture g13 (tests/golden/make_decoder_goldens.py:
HF's SpeechT5ForSpeechToText in fp32 and in float64).  CPU only.  The direct comparison with HF's own modules, where ``transformers``
is importable, is tests/test_decoder_oracle_vs_hf.py.

Bars: a float64 evaluation of the oracle against a float64 evaluation of HF is the same arithmetic in another order, 1e-9 relative
L2 where the fixture keeps float64; the float64 hidden states are stored rounded to fp32 (rounding error 2^-24 = 6e-8 per element),
bar 2e-7.  fp32 against fp32: the suite's first-family bar, 2e-5."""
import numpy as np
import pytest
import torch

import speecht5_decoder_oracle as dec_oracle
from conftest import golden, rel_l2

BAR = 2e-5        # relative L2 between two fp32 evaluations (tests/test_gpu_decoder.py)
BAR_F64 = 1e-9    # between two float64 evaluations
BAR_F64_AS_F32 = 2e-7  # ... one of them stored as fp32
B_PROBE = [5, 12, 23]
B_FRAMES = [149, 97, 1]


@pytest.fixture(scope="module")
def g13():
    return golden("g13_decoder.npz")


def bar64(a):
    assert a.dtype in (np.float32, np.float64), a.dtype
    return BAR_F64 if a.dtype == np.float64 else BAR_F64_AS_F32


def b_enc(synth):
    return (synth.hashed_uniform("g13/enc", (3, 149, 768), 0) * np.float32(1.5)).astype(np.float32)


@pytest.fixture(scope="module")
def a_encoded(synth, oracle, g13, state_dict):
    """The float64 encoder oracle's output for golden A's ragged pair (what _a_inputs of tests/test_gpu_decoder.py builds)."""
    x, m = synth.batch([48000, 30400], first_index=int(g13["a_first_index"]))
    enc = oracle.encode(x, m, state_dict, torch.float64)
    frames = oracle.frame_counts(torch.from_numpy(m), enc.shape[1])
    assert frames.tolist() == g13["a_enc_frames"].tolist()
    return enc, frames


def test_position_ids_match_hf(g13):
    assert dec_oracle.position_ids(torch.from_numpy(g13["b_ids"])).tolist() == g13["b_positions"].tolist()


@pytest.mark.parametrize("dtype,tag", [(torch.float64, "64"), (torch.float32, "32")])
def test_golden_b_forward(synth, g13, dtype, tag):
    sd = synth.decoder_state_dict(int(g13["decoder_seed"]))
    hs = []
    logits = dec_oracle.forward(b_enc(synth), B_FRAMES, g13["b_ids"], sd, dtype, hs)
    assert logits.dtype == dtype and len(hs) == 7
    want_l, want_h = g13["b_logits" + tag], g13["b_hidden" + tag]
    bar_l, bar_h = (bar64(want_l), bar64(want_h)) if tag == "64" else (BAR, BAR)
    r = rel_l2(logits, want_l)
    rh = [rel_l2(h[:, B_PROBE], want_h[l]) for l, h in enumerate(hs)]
    print("golden B", tag, "logits", r, "hidden", rh)
    assert r <= bar_l, r
    assert max(rh) <= bar_h, rh


def test_golden_b_masked_encoder_rows_are_never_read(synth, g13):
    sd = synth.decoder_state_dict(int(g13["decoder_seed"]))
    enc = b_enc(synth)
    want = dec_oracle.forward(enc, B_FRAMES, g13["b_ids"], sd)
    enc[1, 97:] = 1e30
    enc[2, 1:] = 1e30
    assert torch.equal(dec_oracle.forward(enc, B_FRAMES, g13["b_ids"], sd), want)


def test_golden_a_greedy_and_forward(synth, g13, a_encoded):
    enc, frames = a_encoded
    sd = synth.decoder_state_dict(int(g13["decoder_seed"]))
    assert float(g13["a_min_gap"]) >= 1e-3
    ids, steps, lengths, gaps = dec_oracle.greedy(enc, frames, sd, 40)
    assert ids.tolist() == g13["a_ids"].tolist()
    assert lengths.tolist() == g13["a_lengths"].tolist()
    assert steps.shape == (ids.shape[1] - 1, 2, 81) and gaps.shape == steps.shape[:2]
    open_steps = torch.arange(gaps.shape[0])[:, None] + 1 < lengths[None, :]
    assert float(gaps[open_steps].min()) >= 1e-3
    r32, r64 = rel_l2(steps, g13["a_step_logits32"]), rel_l2(steps, g13["a_step_logits64"])
    rf = rel_l2(dec_oracle.forward(enc, frames, g13["a_ids"], sd), g13["a_logits64"])
    print("golden A: step logits vs HF fp32", r32, "vs HF f64", r64, "teacher-forced vs HF f64", rf)
    assert r32 <= BAR, r32
    assert r64 <= bar64(g13["a_step_logits64"]), r64
    assert rf <= bar64(g13["a_logits64"]), rf
    # HF's default length (generate() without a length argument)
    ids_def, _, _, _ = dec_oracle.greedy(enc, frames, sd, g13["a_default_ids"].shape[1])
    assert ids_def.tolist() == g13["a_default_ids"].tolist()


def test_golden_c_early_stop(synth, g13, a_encoded):
    enc, frames = a_encoded
    ids, steps, lengths, _ = dec_oracle.greedy(enc, frames, synth.decoder_state_dict(int(g13["decoder_seed_c"])), 40)
    assert ids.tolist() == g13["c_ids"].tolist()
    assert steps.shape[0] == ids.shape[1] - 1 and int(lengths.max()) == ids.shape[1]


def test_greedy_float32_agrees_with_float64_on_golden_a(synth, g13, a_encoded):
    enc, frames = a_encoded
    sd = synth.decoder_state_dict(int(g13["decoder_seed"]))
    ids, steps, _, _ = dec_oracle.greedy(enc, frames, sd, 40, torch.float32)
    assert ids.tolist() == g13["a_ids"].tolist() and steps.dtype == torch.float32
    assert rel_l2(steps, g13["a_step_logits32"]) <= BAR
