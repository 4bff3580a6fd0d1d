"""CPU tests of the host side of the decoder's output_attentions and of align / align_many: label and head-list errors named before
any launch, which path a forward takes with and without the flag, the C ABI's host-decided error codes and the new symbols."""
import ctypes as C
import importlib
import os
import re

import pytest
import torch

from conftest import ROOT

la = importlib.import_module("loco-asr_amd")
dec = importlib.import_module("loco-asr_amd.decoder")
tr = importlib.import_module("loco-asr_amd.transcribe")
_libmod = importlib.import_module("loco-asr_amd._lib")

NEW_SYMBOLS = ("loco_decoder_forward_attn", "loco_decoder_align_workspace_bytes", "loco_decoder_align", "loco_op_decoder_attention_probs",
               "loco_dtw_align_workspace_bytes", "loco_op_dtw_align")


def small():
    return la.SpeechT5ForSpeechToTextMI355X(layers=1, decoder_layers=2)


def test_align_label_errors_are_named_before_any_launch():
    model = small()
    x = torch.zeros((2, 16000))  # host tensors: anything that got past the checks would fail on "no CPU path" instead
    with pytest.raises(ValueError, match=r"labels\[0, 1\] = -100 is followed by the counted label labels\[0, 3\] = 12"):
        model.align(x, labels=torch.tensor([[5, -100, -100, 12], [7, 2, -100, -100]]))
    with pytest.raises(ValueError, match=r"labels\[1, 0\] = -100 is followed"):
        model.align(x, labels=torch.tensor([[5, 2], [-100, 2]]))
    for labels, match in ((torch.tensor([5, 2]), r"\[batch, tokens\].*batch 2"), (torch.tensor([[5, 81], [7, 2]]), r"labels\[0, 1\] = 81"),
                          (torch.tensor([[0.5, 2.0], [1.0, 2.0]]), "integer token ids"), (torch.zeros((2, 451), dtype=torch.long), "450")):
        with pytest.raises(ValueError, match=match):
            model.align(x, labels=labels)
    with pytest.raises(ValueError, match="needs labels"):
        model.align(x)
    good = torch.tensor([[5, 2], [7, -100]])
    for heads, match in (([], "non-empty"), ([(0, 1, 2)], "pairs"), ([(2, 0)], r"layer 2, head 0.*2 layers x 12 heads"), ([(0, 12)], "head 12"),
                         ([(1, 3), (1, 3)], "twice")):
        with pytest.raises(ValueError, match=match):
            model.align(x, labels=good, alignment_heads=heads)
    with pytest.raises(RuntimeError, match="no CPU path|only on an AMD GPU"):  # valid arguments reach the encoder
        model.align(x, labels=good, alignment_heads=[(1, 11), (0, 0)])
    with pytest.raises(ValueError, match=r"labels\[1\] must be a 1-D tensor"):
        model.align_many([dict(input_values=x)], [torch.tensor([5, 2]), good])
    with pytest.raises(ValueError, match="1 label rows for 2 utterances"):
        model.align_many([dict(input_values=x)], [torch.tensor([5, 2])])
    with pytest.raises(ValueError, match="is followed by the counted label"):
        model.align_many([dict(input_values=x)], [torch.tensor([5, -100, 2]), torch.tensor([5, 2])])
    with pytest.raises(RuntimeError, match="speecht5.decoder"):
        la.SpeechT5ForSpeechToTextMI355X(layers=1).align(x, labels=good)


def test_alignment_counts_and_heads():
    lab = torch.tensor([[5, 9, 2, -100], [-100, -100, -100, -100], [1, 1, 1, 1]])
    assert dec.alignment_counts(lab).tolist() == [3, 0, 4] and dec.alignment_counts(lab).dtype == torch.int32
    assert dec.check_alignment_heads(None, 6) == (None, 0)
    arr, n = dec.check_alignment_heads([(5, 11), (0, 3)], 6)
    assert n == 2 and list(arr) == [5, 11, 0, 3]
    out = dec.TokenAlignment()
    assert [f for f in out.__dataclass_fields__] == ["start_frames", "end_frames", "start_times", "end_times", "attention"]
    assert dec.FRAME_SECONDS == 0.02


def test_forward_takes_the_old_path_without_the_flag(monkeypatch):
    """output_attentions None / False: the encoder call and DecoderRuntime.forward of before; True: the calls that form P.  The other
    refused keywords still raise by name, and generate(output_attentions=) is no parameter of generate."""
    model = small()
    x, ids = torch.zeros((1, 16000)), torch.tensor([[2, 5]])

    class Old(Exception):
        pass

    class New(Exception):
        pass

    def old(*a, **k):
        raise Old

    def new(*a, **k):
        raise New

    monkeypatch.setattr(model, "_encode", old)
    monkeypatch.setattr(model, "_encode_with_attentions", new)
    for flag in (None, False):
        with pytest.raises(Old):
            model(x, decoder_input_ids=ids, output_attentions=flag)
    with pytest.raises(Old):
        model(x, decoder_input_ids=ids)
    with pytest.raises(New):
        model(x, decoder_input_ids=ids, output_attentions=True)
    for kw in ("decoder_attention_mask", "past_key_values", "encoder_outputs", "use_cache"):
        with pytest.raises(NotImplementedError, match=kw):
            model(x, decoder_input_ids=ids, output_attentions=True, **{kw: 1})
    with pytest.raises(TypeError, match="output_attentions"):
        model.generate(x, output_attentions=True)
    out = dec.Seq2SeqLMOutput()
    assert out.decoder_attentions is None and out.cross_attentions is None and out.encoder_attentions is None
    assert [f for f in out.__dataclass_fields__][:5] == ["logits", "encoder_last_hidden_state", "decoder_hidden_states", "loss", "token_logprobs"]


def test_new_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "loco_asr.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(loco_[a-z0-9_]+)\s*\(", text))
    lib = C.CDLL(_libmod.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared and hasattr(lib, name) and name in _libmod.SIGNATURES, name
    # appended: the signatures that were there are what they were
    assert len(_libmod.SIGNATURES["loco_decoder_forward"][1]) == 12 and len(_libmod.SIGNATURES["loco_op_decoder_attention"][1]) == 14
    assert len(_libmod.SIGNATURES["loco_decoder_forward_attn"][1]) == 14


def test_cabi_host_decided_errors():
    lib = _libmod.load()
    buf = (C.c_float * 256)()  # host memory stands in for the pointers: every case below is refused before a launch
    p = C.cast(buf, C.c_void_p)
    assert lib.loco_decoder_align_workspace_bytes(None, 2, 100, 40) == 0
    assert lib.loco_decoder_forward_attn(None, p, None, 1, 1, p, 1, p, None, None, None, p, 1 << 30, None) == -1
    assert b"loco_decoder_forward_attn" in lib.loco_last_error() and b"null encoder" in lib.loco_last_error()
    assert lib.loco_decoder_align(None, p, None, 1, 1, p, 1, p, None, 0, None, p, p, p, 1 << 30, None) == -1
    assert b"loco_decoder_align" in lib.loco_last_error()
    # the DTW operator
    assert lib.loco_dtw_align_workspace_bytes(2, 3, 5) == 30 and lib.loco_dtw_align_workspace_bytes(0, 3, 5) == 0
    assert lib.loco_op_dtw_align(None, 5, p, None, 1, 1, 5, p, p, p, None) == -1 and b"null" in lib.loco_last_error()
    assert lib.loco_op_dtw_align(p, 5, p, None, 1, 451, 5, p, p, p, None) == -1
    assert b"451 tokens exceed the limit of 450" in lib.loco_last_error()
    assert lib.loco_op_dtw_align(p, 4, p, None, 1, 2, 5, p, p, p, None) == -1 and b"ld = 4 < T = 5" in lib.loco_last_error()
    assert lib.loco_op_dtw_align(p, 5, p, None, 0, 2, 5, p, p, p, None) == -1 and b"positive" in lib.loco_last_error()
    # the probabilities operator
    ok = (768, 768, 768, 768)
    assert lib.loco_op_decoder_attention_probs(None, p, None, p, 1, 1, 1, 0, *ok, 0.125, None) == -1 and b"null" in lib.loco_last_error()
    assert lib.loco_op_decoder_attention_probs(p, p, None, p, 1, 0, 1, 0, *ok, 0.125, None) == -1
    assert lib.loco_op_decoder_attention_probs(p, p, None, p, 1, 1, 1, 0, 64, 768, 768, 768, 0.125, None) == -1 and b"768" in lib.loco_last_error()
    assert lib.loco_op_decoder_attention_probs(p, p, None, p, 1, 1, 1, 0, 768, 770, 768, 768, 0.125, None) == -1 and b"multiple of 4" in lib.loco_last_error()


def test_transcribe_timestamp_helpers():
    assert tr.row_length([2, 7, 9, 2, 1, 1]) == 4 and tr.row_length([2, 7, 9]) == 3 and tr.row_length([2, 2, 1]) == 2
    lab = tr.timestamp_labels([[2, 7, 1, 9, 2, 1, 1], [2, 2, 1, 1, 1, 1, 1], [2, 5, 6, 7, 8, 9, 10]])
    assert lab.tolist() == [[7, 1, 9, 2, -100, -100], [2, -100, -100, -100, -100, -100], [5, 6, 7, 8, 9, 10]]  # a <pad> INSIDE a row is a token
    assert dec.alignment_counts(lab).tolist() == [4, 1, 6]
    with pytest.raises(SystemExit, match="exactly one input"):
        tr.main(["--random-init", "--timestamps"])
