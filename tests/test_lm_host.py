"""Host side of the language model: which weight names the C ABI takes, the width it refuses, the CLI's argument surface.  No GPU."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

la = importlib.import_module("loco-asr_amd")
_libmod = importlib.import_module("loco-asr_amd._lib")
eval_ppl = importlib.import_module("loco-asr_amd.eval_ppl")


def set_weight(lib, h, key, shape):
    arr = (C.c_int64 * len(shape))(*shape)
    rc = lib.loco_lm_set_weight(h, key.encode(), None, arr, len(shape))
    return rc, lib.loco_last_error().decode()


def test_key_names_with_and_without_the_prefix():
    lib = _libmod.load()
    h = lib.loco_lm_create(2, 64, 1003, 768, 12)
    assert h
    try:
        # name and shape are judged before the (null) data pointer
        for key, shape in (("transformer.wte.weight", (1003, 768)), ("wte.weight", (1003, 768)), ("transformer.h.1.attn.c_attn.weight", (768, 2304)),
                           ("h.0.mlp.c_proj.weight", (3072, 768)), ("ln_f.bias", (768,))):
            rc, msg = set_weight(lib, h, key, shape)
            assert rc == -1 and "null data" in msg, (key, msg)
        for key in ("transformer.h.0.attn.bias", "h.1.attn.masked_bias", "lm_head.weight"):
            assert set_weight(lib, h, key, (1, 1))[0] == 0, key          # accepted and ignored
        rc, msg = set_weight(lib, h, "transformer.h.2.ln_1.weight", (768,))
        assert rc == -1 and "unknown key" in msg                         # a third block of a 2-layer model
        rc, msg = set_weight(lib, h, "h.0.attn.c_attn.weight", (2304, 768))
        assert rc == -1 and "expected [768, 2304]" in msg                # Conv1D is [in, out]
        buf = C.create_string_buffer(4096)
        assert lib.loco_lm_missing_weights(h, buf, 4096) == 4 + 2 * 12
        assert b"wte.weight" in buf.value and b"h.1.mlp.c_fc.bias" in buf.value
        assert lib.loco_lm_finalize(h, None) == -2                       # LOCO_E_STATE
        assert lib.loco_lm_workspace_bytes(h, 1, 65, 1) == 0 and lib.loco_lm_workspace_bytes(h, 2, 64, 10) > 0
        assert lib.loco_lm_vocab_stride(h) == 1004
    finally:
        lib.loco_lm_destroy(h)


@pytest.mark.parametrize("field, args", [("n_embd", (12, 1024, 50257, 1024, 16)), ("n_head", (12, 1024, 50257, 768, 16)),
                                         ("n_positions", (12, 2048, 50257, 768, 12)), ("n_layer", (0, 1024, 50257, 768, 12))])
def test_unsupported_shapes_are_refused_at_create(field, args):
    lib = _libmod.load()
    assert not lib.loco_lm_create(*args)
    assert field in lib.loco_last_error().decode()
    with pytest.raises(ValueError, match=field):
        la.GPT2LMHeadModelMI355X(*args)


def test_state_dict_surface_and_cpu_refusal():
    sd = la.synth.gpt2_state_dict(0, 1, 8, 64)
    m = la.GPT2LMHeadModelMI355X.from_state_dict(sd)
    assert (m.n_layer, m.n_positions, m.vocab_size) == (1, 8, 64)
    assert set(la.lm.expected_keys(1)) | {"lm_head.weight"} == {la.lm.strip_key(k) for k in sd}
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(torch.zeros(1, 4, dtype=torch.long))
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.token_nll(torch.zeros(1, 4, dtype=torch.long))
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.to("cpu")
    bad = dict(sd)
    del bad["transformer.h.0.ln_2.bias"]
    with pytest.raises(KeyError, match="h.0.ln_2.bias"):
        la.GPT2LMHeadModelMI355X.from_state_dict(bad)
    untied = dict(sd)
    untied["lm_head.weight"] = sd["lm_head.weight"] + np.float32(1)
    with pytest.raises(ValueError, match="tied"):
        la.GPT2LMHeadModelMI355X.from_state_dict(untied)
    with pytest.raises(ValueError, match="n_positions"):
        la.GPT2LMHeadModelMI355X.from_state_dict(sd, n_positions=16)
    import loco_asr_amd
    assert loco_asr_amd.GPT2LMHeadModelMI355X is la.GPT2LMHeadModelMI355X


def test_cli_argument_surface(tmp_path):
    p = eval_ppl.parser()
    a = p.parse_args(["--in_file", "x", "--out_dir", "o", "--random-init", "--layers", "2", "--positions", "32", "--tokenized"])
    assert (a.bsize, a.context_type, a.model, a.strict_reference) == (128, "indep", "gpt2", True)
    a = p.parse_args(["-i", "x", "-o", "o", "--pretrained", "dir", "--ct", "max_len", "--bsize", "5"])
    assert (a.context_type, a.bsize, a.pretrained, a.tokenized) == ("max_len", 5, "dir", False)
    for bad in (["-i", "x", "-o", "o"],                                             # neither --pretrained nor --random-init
                ["-i", "x", "-o", "o", "--random-init", "--model", "gpt2-medium"],  # out of scope
                ["-i", "x", "-o", "o", "--random-init", "--context_type", "full"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    a = p.parse_args(["-i", "x", "-o", "o", "--pretrained", str(tmp_path)])
    with pytest.raises(eval_ppl.TokenizerFilesMissing, match="--tokenized"):
        eval_ppl.load_tokenizer(a, 50257)
    assert "Avg. PPL of recordings: 2.00 std.dev: 1.00 min PPL: 1.00 max PPL: 3.00" == eval_ppl.summary_line({"a": 1.0, "b": 3.0})


def test_from_pretrained_reads_a_checkpoint_directory(tmp_path):
    """config.json + model.safetensors as HF writes them for GPT-2: the tied lm_head.weight is not in the file."""
    import json
    from safetensors.torch import save_file
    sd = la.synth.gpt2_state_dict(0, 1, 8, 64)
    save_file({k: torch.from_numpy(v).contiguous() for k, v in sd.items() if k != "lm_head.weight"}, str(tmp_path / "model.safetensors"))
    (tmp_path / "config.json").write_text(json.dumps({"n_layer": 1, "n_head": 12, "n_embd": 768, "n_positions": 8, "vocab_size": 64,
                                                      "activation_function": "gelu_new"}))
    m = la.GPT2LMHeadModelMI355X.from_pretrained(str(tmp_path))
    assert (m.n_layer, m.n_positions, m.vocab_size) == (1, 8, 64)
    (tmp_path / "config.json").write_text(json.dumps({"n_head": 16}))
    with pytest.raises(ValueError, match="n_head"):
        la.GPT2LMHeadModelMI355X.from_pretrained(str(tmp_path))
