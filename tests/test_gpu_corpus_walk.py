"""score_many and align_many against their hand composition from the public pieces, torch.equal-exactly: the corpus walk (which batches
form a pack, which label rows go with them, the -100 padding to the pack's longest, the per-utterance slices) adds nothing to and takes
nothing from what the packed encoder, the teacher-forced pass, the scoring launch and the alignment compute.

    pytest -m gpu tests/test_gpu_corpus_walk.py
"""
import importlib

import pytest
import torch

import decoder_pool_cases as pc
from test_gpu_decoder_pool import batches_of, small_model

pytestmark = pytest.mark.gpu

IGNORE = -100
LENGTHS = (5, 1, 9, 12, 2, 7)


@pytest.fixture(scope="module")
def gu():
    return importlib.import_module("gpu_util")


@pytest.fixture(scope="module")
def dec():
    return importlib.import_module("loco-asr_amd.decoder")


@pytest.fixture(scope="module")
def corpus(gu):
    """(model, three reference pairs of unequal padded lengths, six label rows that end in </s>)."""
    model = small_model(gu)  # ENC_LAYERS, DEC_LAYERS, DEC_SEED = 2, 2, 13
    oc = pc.oracle_clips(gu.la.synth)
    batches = batches_of(gu, oc[0:4] + oc[10:12])
    assert len({int(b["input_values"].shape[1]) for b in batches}) == 3
    g = torch.Generator().manual_seed(3)
    labels = []
    for n in LENGTHS:
        row = torch.randint(4, 81, (n,), generator=g)
        row[-1] = 2
        labels.append(row)
    return model, batches, labels


def packs_by_hand(model, batches, labels, pack):
    """Per pack of ``pack`` pairs: (packed encoder output, its frame counts, the pack's label rows, those rows padded with -100)."""
    enc = model.speecht5.encoder
    for g0 in range(0, len(batches), pack):
        ticket = enc.forward_packed_async(batches[g0:g0 + pack])
        ticket.result()
        out, _ = ticket.packed_output()
        rows = labels[2 * g0:2 * (g0 + pack)]
        assert out.shape[0] == len(rows)
        lab = torch.full((len(rows), max(len(r) for r in rows)), IGNORE, dtype=torch.long)
        for i, r in enumerate(rows):
            lab[i, :len(r)] = r
        yield out, enc.last_frames, rows, lab


@pytest.mark.parametrize("pack", [1, 2, 3])
def test_score_many_is_its_hand_composition(corpus, dec, pack):
    model, batches, labels = corpus
    want = []
    for out, frames, rows, lab in packs_by_hand(model, batches, labels, pack):
        ids = dec.shift_tokens_right(lab).to(device="cuda", dtype=torch.int32).contiguous()
        logits, _ = model._decoder_runtime.forward(out, frames, ids)
        lp, seq, _, _, _ = dec.score_logits(model.speecht5.encoder._lib, logits, lab.to(device="cuda", dtype=torch.int32).contiguous(), *ids.shape)
        want += [(lp[i, :len(r)].clone(), seq[i].clone()) for i, r in enumerate(rows)]
    got = model.score_many(batches, labels, pack=pack)
    assert len(got) == len(want) == 6
    for u, ((lp, total), (lp0, total0)) in enumerate(zip(got, want)):
        assert lp.shape == (LENGTHS[u],) and total.shape == ()
        assert torch.equal(lp, lp0), (pack, u)
        assert torch.equal(total, total0), (pack, u)


@pytest.mark.parametrize("alignment_heads", [None, [(0, 3), (1, 11)]], ids=["all_heads", "two_layers"])
def test_align_many_is_its_hand_composition(corpus, dec, alignment_heads):
    model, batches, labels = corpus
    heads, pairs = dec.check_alignment_heads(alignment_heads, pc.DEC_LAYERS)
    want = []
    for out, frames, rows, lab in packs_by_hand(model, batches, labels, 2):
        ids = dec.shift_tokens_right(lab).to(device="cuda", dtype=torch.int32).contiguous()
        start, end, A = model._decoder_runtime.align(out, frames, ids, dec.alignment_counts(lab).to("cuda").contiguous(), heads, pairs, True)
        want += [(start[i, :len(r)].clone(), end[i, :len(r)].clone(), A[i, :len(r)].clone()) for i, r in enumerate(rows)]
    got = model.align_many(batches, labels, pack=2, alignment_heads=alignment_heads, return_attention=True)
    assert len(got) == len(want) == 6
    for u, (al, (start, end, A)) in enumerate(zip(got, want)):
        assert al.start_frames.shape == (LENGTHS[u],) and al.attention.shape[0] == LENGTHS[u]
        assert torch.equal(al.start_frames, start) and torch.equal(al.end_frames, end), u
        assert torch.equal(al.start_times, (start.to(torch.float32) * dec.FRAME_SECONDS).to(torch.float32)), u
        assert torch.equal(al.end_times, (end.to(torch.float32) * dec.FRAME_SECONDS).to(torch.float32)), u
        assert torch.equal(al.attention, A), u
        assert bool((start >= 0).all())  # every label of a row counts: none of the times above is the -1 of an ignored one
