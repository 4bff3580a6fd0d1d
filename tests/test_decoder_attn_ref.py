"""CPU: the float64 references of tests/decoder_attn_ref.py are right before the device is measured against them.
1. the restatement with probabilities reproduces the pinned oracle's logits       3. the DTW equals brute-force enumeration of every
2. ... and HF's decoder_attentions / cross_attentions (where transformers imports)    monotone path, all-equal A (the tie rule) included"""
import itertools

import numpy as np
import pytest
import torch

import decoder_attn_ref as ref
import speecht5_decoder_oracle as dec_oracle

SEED = 5


def inputs(synth, B, S, T, tag):
    enc = synth.hashed_uniform(f"dec_attn_ref/{tag}", (B, T, 768), SEED).astype(np.float32)
    ids, _ = synth.token_ids(B, S, seed=SEED)
    ids[:, 0] = 2
    if S > 4:
        ids[0, 2] = 1
        ids[-1, 3:] = 1
    return enc, ids


@pytest.mark.parametrize("B,S,T,frames", [(1, 1, 1, [1]), (4, 9, 70, [65, 64, 63, 1]), (2, 33, 20, None)])
def test_restatement_reproduces_the_oracle(synth, B, S, T, frames):
    sd = synth.decoder_state_dict(SEED)
    enc, ids = inputs(synth, B, S, T, f"{B}/{S}/{T}")
    want = dec_oracle.forward(enc, frames, ids, sd, torch.float64)
    got, p_self, p_cross = ref.forward_with_attentions(enc, frames, ids, sd)
    assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    assert len(p_self) == len(p_cross) == 6
    for ps, pc in zip(p_self, p_cross):
        assert ps.shape == (B, 12, S, S) and pc.shape == (B, 12, S, T)
        assert float((ps.sum(-1) - 1).abs().max()) <= 1e-12 and float((pc.sum(-1) - 1).abs().max()) <= 1e-12
        assert bool((ps.triu(1) == 0).all())  # future keys: exactly 0
        if frames is not None:
            for b, n in enumerate(frames):
                assert bool((pc[b, :, :, n:] == 0).all()) and bool((pc[b, :, :, :n] > 0).all())
    A = ref.mean_attention(p_cross)
    assert A.shape == (B, S, T) and float((A.sum(-1) - 1).abs().max()) <= 1e-12
    sub = ref.mean_attention(p_cross, [(5, 11), (0, 3)])
    assert float((sub - (p_cross[0][:, 3] + p_cross[5][:, 11]) / 2).abs().max()) <= 1e-15


@pytest.mark.parametrize("B,S,T,frames", [(1, 1, 1, [1]), (4, 9, 70, [65, 64, 63, 1]), (2, 33, 20, [20, 7])])
def test_restatement_matches_hf_attentions(synth, B, S, T, frames):
    tr = pytest.importorskip("transformers")
    sd = synth.decoder_state_dict(SEED)
    model = tr.SpeechT5ForSpeechToText(tr.SpeechT5Config()).eval()
    hf_sd = {(k if k.startswith("text_decoder_postnet.") else "speecht5." + k): torch.from_numpy(v) for k, v in sd.items()}
    model.load_state_dict(hf_sd, strict=False)
    model = model.double()
    enc, ids = inputs(synth, B, S, T, f"{B}/{S}/{T}")
    mask = (np.arange(T)[None, :] < np.asarray(frames)[:, None]).astype(np.int64)
    with torch.no_grad():
        r = model.speecht5.decoder(input_values=torch.from_numpy(ids), encoder_hidden_states=torch.from_numpy(enc).double(),
                                   encoder_attention_mask=torch.from_numpy(mask), output_attentions=True)
    _, p_self, p_cross = ref.forward_with_attentions(enc, frames, ids, sd)
    assert len(r.attentions) == len(r.cross_attentions) == 6
    for l in range(6):
        assert float((p_self[l] - r.attentions[l]).abs().max()) <= 1e-9
        assert float((p_cross[l] - r.cross_attentions[l]).abs().max()) <= 1e-9


def monotone_paths(n, F):
    """Every path from (0, 0) to (n-1, F-1) with steps (1,1), (1,0), (0,1), as lists of cells; the moves are enumerated in the order
    that makes the FIRST minimal-cost path the one the tie rule picks when read from the end: see brute_force."""
    def walk(s, t):
        if s == 0 and t == 0:
            yield [(0, 0)]
            return
        for ds, dt in ((1, 1), (1, 0), (0, 1)):  # predecessor: diagonal, then (s-1, t), then (s, t-1)
            if s - ds >= 0 and t - dt >= 0:
                for p in walk(s - ds, t - dt):
                    yield p + [(s, t)]
    return walk(n - 1, F - 1)


def brute_force(A):
    """The cheapest monotone path over -A.  Among equal-cost paths the recurrence's tie rule prefers, at the LAST cell where two of
    them part (walking back from the end), the diagonal predecessor, then (s-1,t), then (s,t-1): ``monotone_paths`` enumerates in that
    preference order (depth first from the end), so the first path with the minimal cost is the rule's path.  Exact float64 sums in
    the recurrence's order (from the origin on), so equal costs compare equal."""
    best, best_cost = None, None
    for p in monotone_paths(*A.shape):
        cost = None
        for s, t in p:
            cost = -A[s, t] if cost is None else -A[s, t] + cost
        if best_cost is None or cost < best_cost:
            best, best_cost = p, cost
    return best


@pytest.mark.parametrize("n,F", list(itertools.product(range(1, 5), range(1, 6))))
def test_dtw_equals_brute_force(n, F):
    rng = np.random.default_rng(1000 * n + F)
    for A in (rng.random((n, F)), np.full((n, F), 0.25), np.zeros((n, F)), np.round(rng.random((n, F)) * 2) / 2):  # random, all equal (twice), many exact ties
        start, end, path = ref.dtw(A)
        assert path == brute_force(np.asarray(A, np.float64)), (n, F, A)
        assert start[0] == 0 and end[n - 1] == F and bool((start < end).all()) and bool((np.diff(start) >= 0).all())
        for s in range(n):
            cells = [t for (i, t) in path if i == s]
            assert start[s] == min(cells) and end[s] == max(cells) + 1


def test_dtw_tie_rule_on_an_all_equal_matrix():
    """The cost is -A: with an all-equal positive A a longer path is cheaper, so no diagonal is taken, and between the two full-length
    ways back from a cell (s-1,t) wins over (s,t-1).  With A == 0 every path costs the same and the diagonal wins wherever it exists."""
    start, end, path = ref.dtw(np.ones((3, 5)))
    assert path == [(0, 0), (0, 1), (0, 2), (0, 3), (0, 4), (1, 4), (2, 4)]
    assert start.tolist() == [0, 4, 4] and end.tolist() == [5, 5, 5]
    start, end, path = ref.dtw(np.ones((4, 2)))
    assert path == [(0, 0), (0, 1), (1, 1), (2, 1), (3, 1)]
    assert start.tolist() == [0, 1, 1, 1] and end.tolist() == [2, 2, 2, 2]
    start, end, path = ref.dtw(np.zeros((3, 5)))
    assert path == [(0, 0), (0, 1), (0, 2), (1, 3), (2, 4)]
    assert start.tolist() == [0, 3, 4] and end.tolist() == [3, 4, 5]
    start, end, path = ref.dtw(np.zeros((4, 2)))
    assert path == [(0, 0), (1, 0), (2, 0), (3, 1)]
    assert start.tolist() == [0, 0, 0, 1] and end.tolist() == [1, 1, 1, 2]


def test_dtw_batch_marks_uncounted_rows():
    A = np.random.default_rng(3).random((3, 4, 6)).astype(np.float32)
    start, end = ref.dtw_batch(A, [4, 0, 2], [6, 6, 3])
    assert (start[1] == -1).all() and (end[1] == -1).all() and start[2].tolist()[2:] == [-1, -1]
    assert end[0, 3] == 6 and end[2, 1] == 3 and start[0, 0] == 0
