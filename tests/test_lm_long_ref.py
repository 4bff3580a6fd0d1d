"""The long-sequence fixture lm4 (tests/golden/make_lm_long_goldens.py: n_positions 1024, sequences of 1024 .. 130 tokens) on the CPU: the
numpy restatement against HuggingFace float64 beyond 64 tokens, the fixture's own consistency, and the condition that makes the GPU tests
of tests/test_gpu_lm_long.py mean something -- an attention fault of one key moves some NLL by at least 10 x the GPU bar."""
import numpy as np
import pytest

import lm_ref
from conftest import golden

LENGTHS = (1024, 700, 341, 300, 257, 130)
_cache = {}


def fixture_and_weights(synth):
    if not _cache:
        g = golden("lm4.npz")
        _cache["lm4"] = (g, synth.gpt2_state_dict(int(g["seed"]), int(g["n_layer"]), int(g["n_positions"]), int(g["vocab"]), float(g["logit_scale"])))
    return _cache["lm4"]


def test_fixture_is_what_it_says():
    g = golden("lm4.npz")
    assert (int(g["n_layer"]), int(g["n_positions"]), int(g["vocab"]), int(g["n_seq"]), int(g["max_len"])) == (2, 1024, 1003, 6, 1024)
    for k, n in enumerate(LENGTHS):
        assert g[f"ids{k}"].shape == (n,) and g[f"nll{k}"].shape == (n - 1,) and g[f"nll{k}"].dtype == np.float64
        assert g[f"ids{k}"].min() >= 0 and g[f"ids{k}"].max() < 1003 and np.isfinite(g[f"nll{k}"]).all()
    # the recording: window 0 in full (targets 1 .. 1023), then the last position of windows 1 .. 5 (targets 1024 .. 1028)
    assert g["rec_ids"].shape == (1030,) and g["rec_nll"].shape == (1028,) and np.isfinite(g["rec_nll"]).all()
    assert g["probe_pos"].tolist() == [0, 63, 64, 255, 256, 511, 512, 1023] and g["probe"].shape == (3, 8, 768) and g["probe"].dtype == np.float64
    assert float(g["logit_std"]) > 2.0
    assert float(g["hf_f64_cached_vs_uncached_max_abs"]) < 1e-12          # one set of NLLs serves the cached and the uncached path
    assert 0 < float(g["hf_fp32_nll_max_abs_err"]) < 1e-3
    assert g["hf_fp32_hidden_rel_l2"].shape == (3,) and g["hf_fp32_hidden_rel_l2"].min() > 0
    assert 4.0 * g["hf_fp32_hidden_rel_l2"].max() <= 2e-5                 # the two hidden-state bars of the GPU tests do not contradict each other


def test_lm_ref_matches_hf_float64_on_300_tokens(synth):
    g, sd = fixture_and_weights(synth)
    err = float(np.abs(lm_ref.token_nll(sd, g["ids3"]) - g["nll3"]).max())
    print("lm4 seq3 (300 tokens) lm_ref vs HF float64", err)
    assert err < 1e-9


def test_recording_windows_are_the_references_walk(synth):
    """The rows stored for the recording are those lm_ref.max_len_batches scores, in its order."""
    g = golden("lm4.npz")
    rec = g["rec_ids"]

    class Tok:
        eos_token_id = int(rec[-1])

        def __call__(self, text):
            return {"input_ids": [int(t) for t in text.split()]}

    batches = lm_ref.max_len_batches([("rec-A-0000-0100", " ".join(map(str, rec[:-1])))], Tok(), 1024, 4)
    targets = []
    for batch, _, first, _ in batches:
        for w in batch:
            o = next(o for o in range(7) if list(rec[o:o + 1024]) == list(w))
            targets += list(range(1, 1024)) if first else [o + 1023]
    assert targets == list(range(1, 1029)) and len(targets) == len(g["rec_nll"])


FAULTS = ["query_300_loses_key_256", "query_200_sees_key_201", "queries_from_257_lose_key_255"]


@pytest.mark.parametrize("fault", FAULTS)
def test_a_planted_attention_fault_moves_the_nll_ten_bars(fault, synth):
    """Sensitivity of the fixture, a condition on the float64 reference alone: on the 341-token sequence each fault -- the size of what a
    wrong tile boundary, an off-by-one causal mask or a dropped key of a split would do -- moves some NLL by at least 10 x the GPU bar
    (4 x hf_fp32_nll_max_abs_err).  If it does not, the fixture is too flat: see the generator's docstring."""
    g, sd = fixture_and_weights(synth)
    ids = g["ids2"]
    S = len(ids)
    assert S == 341
    mask = np.tril(np.ones((S, S), bool))
    if fault == FAULTS[0]:
        mask[300, 256] = False
    elif fault == FAULTS[1]:
        mask[200, 201] = True
    else:
        mask[257:, 255] = False
    if "clean" not in _cache:
        _cache["clean"] = lm_ref.token_nll(sd, ids)
        assert np.abs(_cache["clean"] - g["nll2"]).max() < 1e-9
    moved = float(np.abs(lm_ref.token_nll(sd, ids, mask) - _cache["clean"]).max())
    bar = 4.0 * float(g["hf_fp32_nll_max_abs_err"])
    print(fault, "moves the NLL by", moved, "=", moved / bar, "x the GPU bar", bar)
    assert moved >= 10.0 * bar
