"""The float64 restatement (tests/lm_ref.py) against HuggingFace's own GPT2LMHeadModel run in float64 (fixtures lm1 / lm2, written by
tests/golden/make_lm_goldens.py): NLLs and the hidden states' probe rows at float64 round-off.  CPU only."""
import numpy as np
import pytest

import lm_ref
from conftest import golden

_cache = {}


def fixture_and_weights(name, synth):
    if name not in _cache:
        g = golden(name + ".npz")
        sd = synth.gpt2_state_dict(int(g["seed"]), int(g["n_layer"]), int(g["n_positions"]), int(g["vocab"]), float(g["logit_scale"]))
        _cache[name] = (g, sd)
    return _cache[name]


@pytest.mark.parametrize("name", ["lm1", "lm2"])
def test_lm_ref_matches_hf_float64(name, synth):
    g, sd = fixture_and_weights(name, synth)
    assert float(g["logit_std"]) > 2.0                      # a softmax that is far from flat
    assert sd["lm_head.weight"] is sd["transformer.wte.weight"]
    worst_nll = worst_h = 0.0
    for k in range(int(g["n_seq"])):
        ids = g[f"ids{k}"]
        hs = lm_ref.hidden_states(sd, ids)
        assert len(hs) == int(g["n_layer"]) + 1
        nll = lm_ref.head_nll(hs[-1][:-1], sd["transformer.wte.weight"], ids[1:])
        worst_nll = max(worst_nll, float(np.abs(nll - g[f"nll{k}"]).max()))
        probe, pos = g[f"probe{k}"], g[f"probe_pos{k}"]
        for i, h in enumerate(hs):
            worst_h = max(worst_h, float(np.linalg.norm(h[pos] - probe[i]) / np.linalg.norm(probe[i])))
    print(name, "nll", worst_nll, "hidden", worst_h)
    # float64 on both sides, sums of up to 50 257 terms in different orders: 1e-10 is 1e5 x below what the fp32 paths are judged by
    assert worst_nll < 1e-10 and worst_h < 1e-12


def test_hf_fp32_figures_are_recorded():
    for name in ("lm1", "lm2"):
        g = golden(name + ".npz")
        assert 0 < float(g["hf_fp32_nll_max_abs_err"]) < 1e-3
        assert g["hf_fp32_hidden_rel_l2"].shape == (int(g["n_layer"]) + 1,) and 0 < g["hf_fp32_hidden_rel_l2"].max() < 2e-5


def test_gelu_new_forms_agree():
    x = np.linspace(-12, 12, 4001)
    u = np.sqrt(2 / np.pi) * (x + 0.044715 * x ** 3)
    with np.errstate(over="ignore"):
        sig = x / (1.0 + np.exp(-2.0 * u))     # the form csrc/loco_kernels.h evaluates
    assert np.abs(lm_ref.gelu_new(x) - sig).max() < 1e-15
