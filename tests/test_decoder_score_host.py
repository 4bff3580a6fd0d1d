"""CPU tests of the scoring path's host side (forward(labels=), score, generate(output_scores=), loco_decoder_score's argument
checks, decoder.shift_tokens_right) and of the reference the GPU tests hold the loss to: HuggingFace's labels= loss against
F.cross_entropy of the float64 decoder oracle's logits."""
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import speecht5_decoder_oracle as dec_oracle

la = importlib.import_module("loco-asr_amd")
dec = importlib.import_module("loco-asr_amd.decoder")
_libmod = importlib.import_module("loco-asr_amd._lib")
synth = la.synth

LABELS = torch.tensor([[5, 9, -100, 12, 2, -100, -100],    # -100 inside the row and over its tail
                       [80, 0, 7, 7, 30, 41, 2],
                       [-100, -100, -100, -100, -100, -100, -100]])


def test_labels_on_an_encoder_only_model_name_the_missing_decoder():
    model = la.SpeechT5ForSpeechToTextMI355X(layers=1)
    x = torch.zeros((1, 16000))
    with pytest.raises(RuntimeError, match="text_decoder_postnet.lm_head.weight"):
        model(x, labels=torch.tensor([[5, 2]]))
    with pytest.raises(RuntimeError, match="speecht5.decoder"):
        model.score(x, labels=torch.tensor([[5, 2]]))
    with pytest.raises(RuntimeError, match="speecht5.decoder"):
        model.score_many([dict(input_values=x)], [torch.tensor([5, 2])])


def test_label_errors_are_named_before_any_launch():
    model = la.SpeechT5ForSpeechToTextMI355X(layers=1, decoder_layers=1)
    x = torch.zeros((2, 16000))  # host tensors: anything that got past the checks would fail on "no CPU path" instead
    good = torch.tensor([[5, 2], [7, -100]])
    for labels, match in ((torch.tensor([5, 2]), r"\[batch, tokens\].*batch 2"), (good[:1], "batch 2"),
                          (torch.tensor([[5, 81], [7, 2]]), r"labels\[0, 1\] = 81"), (torch.tensor([[5, 2], [-1, 2]]), r"labels\[1, 0\] = -1"),
                          (torch.tensor([[0.5, 2.0], [1.0, 2.0]]), "integer token ids"), (torch.zeros((2, 451), dtype=torch.long), "450")):
        with pytest.raises(ValueError, match=match):
            model(x, labels=labels)
        with pytest.raises(ValueError, match=match):
            model.score(x, labels=labels)
    with pytest.raises(ValueError, match=r"labels \(2, 2\) and decoder_input_ids \(2, 3\)"):
        model(x, labels=good, decoder_input_ids=torch.tensor([[2, 5, 9], [2, 7, 1]]))
    with pytest.raises(ValueError, match=r"labels\[1\] must be a 1-D tensor"):
        model.score_many([dict(input_values=x)], [torch.tensor([5, 2]), good])
    with pytest.raises(ValueError, match="1 label rows for 2 utterances"):
        model.score_many([dict(input_values=x)], [torch.tensor([5, 2])])
    with pytest.raises(ValueError, match="needs labels"):
        model.score(x)
    with pytest.raises(RuntimeError, match="no CPU path|only on an AMD GPU"):  # valid labels reach the encoder
        model(x, labels=good)
    # the names that raised before labels= was implemented still do
    with pytest.raises(NotImplementedError, match="decoder_attention_mask"):
        model(x, labels=good, decoder_attention_mask=torch.ones(2, 2))
    with pytest.raises(TypeError, match="bogus"):
        model(x, labels=good, bogus=1)


def test_generate_score_arguments():
    model = la.SpeechT5ForSpeechToTextMI355X(layers=1, decoder_layers=1)
    x = torch.zeros((1, 16000))
    with pytest.raises(TypeError, match="bogus"):
        model.generate(x, output_scores=True, bogus=1)
    with pytest.raises(TypeError, match="bogus"):
        model.generate(x, output_scores=True, return_dict_in_generate=True, bogus=1)
    with pytest.raises(NotImplementedError, match="num_beams"):
        model.generate(x, output_scores=True, return_dict_in_generate=True, num_beams=4)
    with pytest.raises(TypeError, match="bogus"):
        model.generate_many([dict(input_values=x)], return_scores=True, bogus=1)
    with pytest.raises(RuntimeError, match="no CPU path|only on an AMD GPU"):  # both names are parameters: the call reaches the encoder
        model.generate(x, output_scores=True, return_dict_in_generate=True)
    out = dec.Seq2SeqLMOutput()
    assert out.loss is None and out.token_logprobs is None
    assert [f for f in out.__dataclass_fields__][:3] == ["logits", "encoder_last_hidden_state", "decoder_hidden_states"]


def test_cabi_score_argument_errors_need_no_device():
    lib = _libmod.load()
    none = (None,) * 5
    assert lib.loco_decoder_score(None, 81, None, 1, 1, 81, -100, None, *none) == -1
    assert b"loco_decoder_score" in lib.loco_last_error() and b"null" in lib.loco_last_error()
    import ctypes as C
    buf = (C.c_float * 128)()  # host memory stands in for the pointers: every case below is refused before a launch
    p = C.cast(buf, C.c_void_p)
    assert lib.loco_decoder_score(p, 81, None, 1, 1, 81, -100, None, *none) == -1
    for B, S, V, ld, word in ((0, 1, 81, 81, b"B = 0"), (1, 0, 81, 81, b"S = 0"), (1, 1, 0, 81, b"V = 0"), (1, 1, 81, 80, b"ld = 80 < V = 81"),
                              (65536, 65536, 81, 81, b"2^31")):
        assert lib.loco_decoder_score(p, ld, None, B, S, V, -100, p, *none) == -1, (B, S, V, ld)
        assert word in lib.loco_last_error(), lib.loco_last_error()


def test_shift_tokens_right():
    got = dec.shift_tokens_right(LABELS)
    want = torch.full_like(LABELS, 0)   # the three-line restatement
    want[:, 0], want[:, 1:] = 2, LABELS[:, :-1]
    want[want == -100] = 1
    assert got.tolist() == want.tolist() and got.dtype == LABELS.dtype
    assert got[0].tolist() == [2, 5, 9, 1, 12, 2, 1] and got[2].tolist() == [2, 1, 1, 1, 1, 1, 1]
    assert LABELS[0, 2] == -100  # the argument is left as it was
    assert dec.shift_tokens_right(torch.tensor([[7]])).tolist() == [[2]]


def test_shift_tokens_right_equals_hf():
    hf = pytest.importorskip("transformers.models.speecht5.modeling_speecht5")
    assert dec.shift_tokens_right(LABELS).tolist() == hf.shift_tokens_right(LABELS.clone(), 1, 2).tolist()


def test_hf_loss_is_cross_entropy_of_the_oracle_logits():
    """The reference of the GPU tests' loss: HF's own labels= loss (1 + 1 layers, float64) against F.cross_entropy of the float64
    decoder oracle's logits on the ids decoder.shift_tokens_right makes of the labels, both on HF's encoder output."""
    tr = pytest.importorskip("transformers")
    seed = 5
    enc_sd, dec_sd = synth.encoder_state_dict(seed, 1), synth.decoder_state_dict(seed, 1)
    model = tr.SpeechT5ForSpeechToText(tr.SpeechT5Config(encoder_layers=1, decoder_layers=1)).eval()
    hf_sd = {"speecht5.encoder." + k: torch.from_numpy(v) for k, v in enc_sd.items()}
    hf_sd.update({(k if k.startswith("text_decoder_postnet.") else "speecht5." + k): torch.from_numpy(v) for k, v in dec_sd.items()})
    missing, unexpected = model.load_state_dict(hf_sd, strict=False)
    assert not unexpected and all("embed_positions" in k for k in missing), (missing, unexpected)
    model = model.double()
    x, m = synth.batch([8000, 4800, 6400], first_index=30)
    xs, ms = torch.from_numpy(x).double(), torch.from_numpy(m).long()
    with torch.no_grad():
        out = model(input_values=xs, attention_mask=ms, labels=LABELS)
    enc_out = out.encoder_last_hidden_state
    frames = model.speecht5.encoder.prenet._get_feature_vector_attention_mask(enc_out.shape[1], ms).sum(1)
    assert frames.tolist()[0] == enc_out.shape[1] and frames.tolist()[1] < enc_out.shape[1]
    logits = dec_oracle.forward(enc_out, frames, dec.shift_tokens_right(LABELS), dec_sd, torch.float64)
    assert float((logits - out.logits).abs().max() / out.logits.abs().max()) <= 1e-9
    want = F.cross_entropy(logits.reshape(-1, logits.shape[-1]), LABELS.reshape(-1))  # ignore_index -100, mean over the rest
    assert np.isfinite(float(out.loss)) and abs(float(out.loss) - float(want)) <= 1e-9, (float(out.loss), float(want))
    # the per-token form the GPU tests use: -(sum of log_softmax at the labels that count) / their number
    lp = torch.log_softmax(logits, -1).gather(-1, LABELS.clamp(min=0)[..., None])[..., 0] * (LABELS != -100)
    assert abs(float(-lp.sum() / (LABELS != -100).sum()) - float(out.loss)) <= 1e-9
