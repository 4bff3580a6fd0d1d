"""CPU tests of the decoder's host side: key surface, the position-id rule, checkpoint loading with the tied weight present once,
generate's argument handling, the C ABI's host-only answers, and the self-consistency of tests/golden/g13_decoder.npz."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

from conftest import golden

la = importlib.import_module("loco-asr_amd")
dec = importlib.import_module("loco-asr_amd.decoder")
_libmod = importlib.import_module("loco-asr_amd._lib")
synth = la.synth


def _t(d):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in d.items()}


def _full_state_dict(layers=1, dec_layers=1):
    sd = {"speecht5.encoder." + k: v for k, v in synth.encoder_state_dict(0, layers).items()}
    for k, v in synth.decoder_state_dict(0, dec_layers).items():
        sd[k if k.startswith("text_decoder_postnet.") else "speecht5." + k] = v
    return sd


def test_key_surface_matches_hf_and_synth():
    g = golden("g13_decoder.npz")
    hf = {str(k): tuple(int(d) for d in str(s).split(",")) for k, s in zip(g["decoder_keys"], g["decoder_shapes"])}
    sy = synth.decoder_state_dict(0)
    mine = {(k if k.startswith("text_decoder_postnet.") else "speecht5." + k): tuple(v.shape) for k, v in sy.items()}
    assert mine == hf
    assert len(hf) == 158
    model = la.SpeechT5ForSpeechToTextMI355X(layers=1, decoder_layers=6)
    mod = {"speecht5.decoder." + k: tuple(v.shape) for k, v in model.speecht5.decoder.state_dict().items()}
    mod.update({"text_decoder_postnet." + k: tuple(v.shape) for k, v in model.text_decoder_postnet.state_dict().items()})
    assert mod == hf
    # the encoder's own modules are untouched by the decoder's presence
    enc_keys = set("prenet." + k for k in model.speecht5.encoder.prenet.state_dict()) | set(
        "wrapped_encoder." + k for k in model.speecht5.encoder.wrapped_encoder.state_dict())
    assert enc_keys == set(synth.encoder_state_dict(0, 1))
    assert sy["text_decoder_postnet.lm_head.weight"] is sy["decoder.prenet.embed_tokens.weight"]


def test_position_ids_rule():
    g = golden("g13_decoder.npz")
    ids = torch.from_numpy(g["b_ids"])
    assert bool((ids == 1).any()) and int(ids[0, 5]) == 1  # <pad> inside a row
    assert dec.position_ids(ids).tolist() == g["b_positions"].tolist()
    assert dec.position_ids(torch.tensor([[7]]), 5).tolist() == [[7]]  # the cached step: (1 + past) * mask + 1
    tab = la.sinusoid_table(452)
    assert tab.shape == (452, 768) and bool((tab[1] == 0).all())


@pytest.mark.parametrize("fmt", ["safetensors", "bin"])
def test_from_pretrained_keeps_decoder(tmp_path, fmt):
    sd = _t(_full_state_dict())
    del sd["text_decoder_postnet.lm_head.weight"]  # tie_word_embeddings: the tied tensor is stored once
    if fmt == "safetensors":
        from safetensors.torch import save_file
        save_file({k: v.contiguous() for k, v in sd.items()}, str(tmp_path / "model.safetensors"))
    else:
        torch.save(sd, str(tmp_path / "pytorch_model.bin"))
    model = la.SpeechT5ForSpeechToTextMI355X.from_pretrained(str(tmp_path))
    assert model.has_decoder and model.speecht5.decoder.num_layers == 1
    assert torch.equal(model.text_decoder_postnet.lm_head.weight, sd["speecht5.decoder.prenet.embed_tokens.weight"])
    assert torch.equal(model.speecht5.decoder.state_dict()["wrapped_decoder.layers.0.encoder_attn.k_proj.weight"],
                       sd["speecht5.decoder.wrapped_decoder.layers.0.encoder_attn.k_proj.weight"])


def test_encoder_only_checkpoint_still_loads_and_generate_raises(tmp_path):
    sd = {k: v for k, v in _t(_full_state_dict()).items() if k.startswith("speecht5.encoder.")}
    torch.save(sd, str(tmp_path / "pytorch_model.bin"))
    model = la.SpeechT5ForSpeechToTextMI355X.from_pretrained(str(tmp_path))
    assert not model.has_decoder and not hasattr(model.speecht5, "decoder")
    x = torch.zeros((1, 16000))
    with pytest.raises(RuntimeError, match="text_decoder_postnet.lm_head.weight"):
        model.generate(x)
    with pytest.raises(RuntimeError, match="speecht5.decoder"):
        model(x, decoder_input_ids=torch.tensor([[2]]))


def test_decoder_missing_tensor_is_named():
    pre, enc = synth.split_state_dict(synth.encoder_state_dict(0, 1))
    d, p = synth.split_decoder_state_dict(synth.decoder_state_dict(0, 1))
    del d["wrapped_decoder.layers.0.encoder_attn.v_proj.bias"]
    with pytest.raises(RuntimeError, match="encoder_attn.v_proj.bias"):
        la.SpeechT5ForSpeechToTextMI355X.from_state_dicts(_t(pre), _t(enc), layers=1, decoder_state_dict=_t(d), postnet_state_dict=_t(p))


def test_generate_arguments():
    model = la.SpeechT5ForSpeechToTextMI355X(layers=1, decoder_layers=1)
    x = torch.zeros((1, 16000))
    for kw in (dict(num_beams=4), dict(do_sample=True), dict(decoder_attention_mask=torch.ones(1, 1)), dict(decoder_input_ids=torch.tensor([[2, 5]])),
               dict(temperature=0.7)):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            model.generate(x, **kw)
    with pytest.raises(TypeError, match="bogus"):
        model.generate(x, bogus=1)
    with pytest.raises(ValueError, match="450"):
        model.generate(x, max_length=451)
    assert dec.resolve_max_length(None, None) == golden("g13_decoder.npz")["a_default_ids"].shape[1]  # one row of A never ends
    assert dec.resolve_max_length(100, None) == 100 and dec.resolve_max_length(100, 7) == 8
    with pytest.raises(NotImplementedError, match="decoder_attention_mask"):
        model(x, decoder_input_ids=torch.tensor([[2]]), decoder_attention_mask=torch.ones(1, 1))


def test_cabi_host_only_answers():
    """What the C ABI answers without touching a device: sizes, and the state / argument errors that are decided before any launch."""
    lib = _libmod.load()
    assert lib.loco_decoder_max_batch() == 64
    assert lib.loco_has_decoder(None) == 0
    assert lib.loco_decoder_workspace_bytes(None, 2, 100, 40) == 0
    for fn, args in (("loco_decoder_begin", (None, None, None, 2, 100, 40, None, 0, None)),
                     ("loco_decoder_step", (None, 2, 100, 40, 0, None, None, 0, None))):
        assert getattr(lib, fn)(*args) == -1  # LOCO_E_INVALID: null handle
    assert lib.loco_decoder_attention_scratch_bytes(1, 1, 29999) > 0  # a long key range is split
    assert lib.loco_decoder_attention_scratch_bytes(3, 450, 450) == 0  # enough rows: no split
    a = lib.loco_decoder_attention_scratch_bytes
    assert a(1, 1, 64) <= a(1, 1, 1499) <= a(1, 1, 29999)
    assert lib.loco_op_skinny_gemm(None, 768, None, 768, None, None, 0, None, 768, 2, 8, 768, 0, None) == -1


def test_golden_self_consistency():
    g = golden("g13_decoder.npz")
    ids, steps, lengths = g["a_ids"], g["a_step_logits32"], g["a_lengths"]
    B, S = ids.shape
    assert steps.shape == (S - 1, B, 81) and (ids[:, 0] == 2).all()
    assert (lengths < 40).any() and (lengths == 40).any()  # condition (ii)
    for b in range(B):
        done = False
        for t in range(S - 1):
            want = 1 if done else int(np.argmax(steps[t, b]))
            assert int(ids[b, t + 1]) == want, (b, t)
            done = done or want == 2
        assert int(lengths[b]) == (int(np.argmax(ids[b, 1:] == 2)) + 2 if (ids[b, 1:] == 2).any() else S)
    assert float(g["a_min_gap"]) >= 1e-3       # condition (i)
    assert float(g["a_cached_vs_uncached"]) < 2e-5  # condition (iii)
    d = g["a_default_ids"]
    assert d.shape[1] <= 40 and (d == ids[:, :d.shape[1]]).all()
    c = g["c_ids"]  # case C: every row ends, HF stops there
    assert c.shape[1] < 40 and (c[:, 0] == 2).all() and (c[:, 1:] == 2).any(axis=1).all() and (c[:, -1] == 2).any()


# ---- transcribe.py: everything that needs no device ---------------------------------------------------------------------------
tr = importlib.import_module("loco-asr_amd.transcribe")


def _args(**kw):
    import argparse
    base = dict(split=None, files=[], synthetic=0, synthetic_seconds=5.0, data_path="slurp")
    base.update(kw)
    return argparse.Namespace(**base)


def _write_wav(path, x, rate=16000):
    import wave
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes((np.clip(x, -1, 1) * 32767).astype("<i2").tobytes())


def test_transcribe_strip_special_and_tokenizer_lookup(tmp_path):
    assert tr.strip_special([2, 7, 9, 1, 12, 2, 1, 1]) == [7, 9, 12]  # start token dropped, <pad> skipped, stops at </s>
    assert tr.strip_special([2, 2, 1, 1]) == [] and tr.strip_special([2, 5, 6]) == [5, 6]
    assert tr.load_tokenizer(None) is None
    assert tr.load_tokenizer(str(tmp_path / "nowhere")) is None          # nothing on disk: no "text", and nothing is fetched
    assert tr.load_tokenizer("microsoft/speecht5_asr") is None           # a hub name is not looked up anywhere
    (tmp_path / "tok").mkdir()
    assert tr.load_tokenizer(str(tmp_path / "tok")) is None              # a directory without spm_char.model


def test_transcribe_input_sources(tmp_path):
    with pytest.raises(SystemExit, match="exactly one input"):
        tr.gather_items(_args())
    with pytest.raises(SystemExit, match="exactly one input"):
        tr.gather_items(_args(synthetic=2, files=["a.wav"]))
    items = tr.gather_items(_args(synthetic=3, synthetic_seconds=1.0))
    assert [i[0] for i in items] == ["synthetic-000000", "synthetic-000001", "synthetic-000002"] and all(p is None and n > 0 for _, p, n in items)
    assert tr.gather_items(_args(files=["/x/b.flac", "/y/a.wav"])) == [("b", "/x/b.flac", 0), ("a", "/y/a.wav", 0)]  # the order given
    # a SLURP split through extract.py's reader: corpus order, headset recording preferred
    import json
    (tmp_path / "dataset" / "slurp").mkdir(parents=True)
    (tmp_path / "audio" / "slurp_real").mkdir(parents=True)
    rows = [dict(slurp_id=9, sentence="wake me", intent="alarm_set", recordings=[{"file": "a-far.wav"}, {"file": "a-headset.wav", "headset": True}]),
            dict(slurp_id=4, sentence="stop", intent="audio_volume_mute", recordings=[{"file": "b.wav"}])]
    with open(tmp_path / "dataset" / "slurp" / "devel.jsonl", "w") as fh:
        fh.write("\n".join(json.dumps(r) for r in rows) + "\n")
    got = tr.gather_items(_args(split="devel", data_path=str(tmp_path)))
    audio = str(tmp_path / "audio" / "slurp_real")
    assert got == [("9", audio + "/a-headset.wav", 0), ("4", audio + "/b.wav", 0)]
    # one reference batch of two files: decoded, padded to the longest, masked
    xa, xb = synth.clip(0, 16000), synth.clip(1, 9600)
    _write_wav(tmp_path / "audio" / "slurp_real" / "a-headset.wav", xa)
    _write_wav(tmp_path / "audio" / "slurp_real" / "b.wav", xb)
    f = tr.load_batch(got, 0, la.SpeechT5FeatureExtractorMI355X(), None)
    assert tuple(f["input_values"].shape) == (2, 16000) and f["attention_mask"].sum(dim=1).tolist() == [16000, 9600]
    assert float((f["input_values"][1, :9600] - torch.from_numpy(xb)).abs().max()) < 1e-4 and bool((f["input_values"][1, 9600:] == 0).all())
    s = tr.load_batch(tr.gather_items(_args(synthetic=2, synthetic_seconds=1.0)), 0, la.SpeechT5FeatureExtractorMI355X(), None)
    assert s["input_values"].shape[0] == 2 and int(s["attention_mask"][0].sum()) > 0


def test_transcribe_argument_errors():
    with pytest.raises(SystemExit, match="exactly one input"):
        tr.main(["--random-init"])
    with pytest.raises(SystemExit, match="--pretrained DIR or --random-init"):
        tr.main(["--synthetic", "2"])
    with pytest.raises(SystemExit, match="batch-size"):
        tr.main(["--random-init", "--synthetic", "2", "--batch-size", "0"])
