"""The n-gram language model on the GPU (csrc/ngram.hip, csrc/ngram_api.hip) against tests/ngram_ref.py.

1. loco_op_ngram_logprobs, bit for bit (the doubles compared as int64): orders 1, 2, 5, 8; V = 5, 81, 127; rows that hold the start
   token alone, fewer than order - 1 tokens and at least order - 1; contexts that were seen, wholly unseen ones and ones with an unseen
   id in the middle; one table of more than 50 000 grams, so that probe sequences are longer than one slot.  The output sits between
   guard bands, the row stride is longer than the rows.
2. Row independence: a row run alone and run among 64 rows gives the same bits.
3. loco_op_ngram_score against the restatement per token; NgramLM's own methods on top of both.
4. loco_ngram_create's refusals: LOCO_E_INVALID naming the gram or the field.
The rule is this project's own: it is NOT validated against KenLM/SRILM binaries.
"""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import fusion_cases as fc
import ngram_ref as ng
from test_gpu_decoder_beam import Guarded, same_bits

pytestmark = pytest.mark.gpu

_tables = {}


@pytest.fixture(scope="module")
def gu():
    return importlib.import_module("gpu_util")


def as_p(a):
    return a.ctypes.data_as(C.c_void_p)


def create(gu, V, order, lengths, symbols, logp, backoff):
    """(return code, handle) of loco_ngram_create on host arrays."""
    out = C.c_void_p()
    lengths, symbols = np.ascontiguousarray(lengths, np.int32), np.ascontiguousarray(symbols, np.int32)
    logp, backoff = np.ascontiguousarray(logp, np.float64), np.ascontiguousarray(backoff, np.float64)
    rc = gu.lib().loco_ngram_create(V, order, len(lengths), as_p(lengths), as_p(symbols), as_p(logp), as_p(backoff), C.byref(out))
    return rc, out


def table(gu, order, V, sentences=200, ids=None, seed=None):
    """(the restatement's model, the device handle, the corpus), built once per (order, V, size)."""
    key = (order, V, sentences)
    if key not in _tables:
        ids = ids or range(3, max(V - 3, 4))  # the last three ids stay unseen where the vocabulary has room
        seqs = ng.corpus(order * 1000 + V if seed is None else seed, sentences, ids, length=(3, 14))
        m = ng.train(seqs, order, V)
        rc, h = create(gu, V, order, *ng.arrays(m))
        gu.check(rc, "loco_ngram_create")
        _tables[key] = (m, h, seqs)
    return _tables[key]


def device_logprobs(gu, handle, V, rows, pad=3):
    """loco_op_ngram_logprobs on token rows of different lengths: f64 [R, V] from between guard bands."""
    S = max(len(r) for r in rows)
    tok = np.full((len(rows), S + pad), -9, np.int32)  # behind a row's tokens, and in the stride's slack: never read
    for i, r in enumerate(rows):
        tok[i, :len(r)] = r
    t, cur = Guarded(tok), Guarded(np.array([len(r) for r in rows], np.int32))
    out = Guarded(np.full((len(rows), V), 7.25, np.float64))
    gu.check(gu.lib().loco_op_ngram_logprobs(handle, t.ptr, S + pad, S, cur.ptr, len(rows), out.ptr, gu.stream()), "loco_op_ngram_logprobs")
    torch.cuda.synchronize()
    assert same_bits(t.back(), tok)
    return out.back()


def rows_for(seqs, order, V):
    rows = [r for kind in fc.probe_rows(seqs, order, V).values() for r in kind]
    return [[min(t, V - 1) for t in r] for r in rows]


# ---- 1. next-token log-probabilities ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [5, 81, 127])
@pytest.mark.parametrize("order", [1, 2, 5, 8])
def test_logprobs_match_the_restatement_bit_for_bit(gu, order, V):
    m, h, seqs = table(gu, order, V, ids=range(3, 5) if V == 5 else None)
    rows = rows_for(seqs, order, V)
    assert any(len(r) == 1 for r in rows) and any(len(r) >= order - 1 for r in rows) and (order < 4 or any(1 < len(r) < order - 1 for r in rows))
    got = device_logprobs(gu, h, V, rows)
    want = np.stack([ng.next_logprobs(m, r) for r in rows])
    assert same_bits(got.view(np.int64), want.view(np.int64)), np.argwhere(got.view(np.int64) != want.view(np.int64))[:5]
    assert float(np.abs(np.exp(got).sum(1) - 1).max()) <= 1e-12


def test_a_large_table_with_probe_chains(gu):
    """More than 50 000 grams at load factor <= 0.5: some keys do not sit in their first slot, so the probe loop runs."""
    m, h, seqs = table(gu, 6, 81, sentences=4000)
    assert len(m.logp) >= 50000, len(m.logp)
    rows = rows_for(seqs, 6, 81) + [[2] + s for s in seqs[:40]]
    got = device_logprobs(gu, h, 81, rows)
    want = np.stack([ng.next_logprobs(m, r) for r in rows])
    assert same_bits(got.view(np.int64), want.view(np.int64))


def test_rows_outside_the_rule_are_nan(gu):
    m, h, _ = table(gu, 5, 81)
    tok = torch.tensor([[2, 5, 6, 0], [2, 5, 81, 7], [2, 5, -1, 7], [2, 5, 6, 7]], dtype=torch.int32, device="cuda")
    cur = torch.tensor([0, 4, 4, 5], dtype=torch.int32, device="cuda")  # no tokens; an id >= V; a negative id; more tokens than S
    out = torch.zeros((4, 81), dtype=torch.float64, device="cuda")
    gu.check(gu.lib().loco_op_ngram_logprobs(h, gu.ptr(tok), 4, 4, gu.ptr(cur), 4, gu.ptr(out), gu.stream()), "loco_op_ngram_logprobs")
    assert bool(torch.isnan(out).all())
    lib = gu.lib()
    assert lib.loco_op_ngram_logprobs(h, gu.ptr(tok), 3, 4, gu.ptr(cur), 4, gu.ptr(out), gu.stream()) == -1 and "ld" in lib.loco_last_error().decode()
    assert lib.loco_op_ngram_logprobs(None, gu.ptr(tok), 4, 4, gu.ptr(cur), 4, gu.ptr(out), gu.stream()) == -1


# ---- 2. row independence -----------------------------------------------------------------------------------------------------------------
def test_a_row_alone_and_among_64_rows(gu):
    m, h, seqs = table(gu, 5, 81)
    rows = ([[2] + s for s in seqs] + rows_for(seqs, 5, 81))[:64]
    assert len(rows) == 64
    together = device_logprobs(gu, h, 81, rows)
    for i in range(64):
        alone = device_logprobs(gu, h, 81, [rows[i]], pad=0)
        assert same_bits(alone[0].view(np.int64), together[i].view(np.int64)), i
    shuffled = device_logprobs(gu, h, 81, rows[::-1])
    assert same_bits(shuffled[::-1].view(np.int64), together.view(np.int64))


# ---- 3. teacher-forced scores ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 3, 8])
def test_score_matches_the_restatement_per_token(gu, order):
    m, h, seqs = table(gu, order, 81)
    hyps = [[2] + s + [2] for s in seqs[:20]] + [[2], [2, 2], [2, 80, 79, 5, 6, 2], [2] + seqs[0] * 30]  # the last: 256 threads, a second round
    lens = np.array([len(x) for x in hyps], np.int32)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    flat = np.concatenate([np.array(x, np.int32) for x in hyps])
    t, st, ln = Guarded(flat), Guarded(starts), Guarded(lens)
    out = Guarded(np.full(flat.shape[0], 7.25, np.float64))
    gu.check(gu.lib().loco_op_ngram_score(h, t.ptr, flat.shape[0], st.ptr, ln.ptr, len(hyps), out.ptr, gu.stream()), "loco_op_ngram_score")
    torch.cuda.synchronize()
    got = out.back()
    for a, x in zip(starts.tolist(), hyps):
        want = ng.token_logprobs(m, x)
        assert same_bits(got[a:a + len(x)].view(np.int64), want.view(np.int64)), x[:8]


def test_ngramlm_methods(gu, tmp_path):
    P = importlib.import_module("loco-asr_amd.ngram")
    seqs = fc.fusion_corpus()
    m = fc.fusion_model()
    lm = P.NgramLM.train(seqs, fc.LM_ORDER, fc.V_MODEL)
    with pytest.raises(RuntimeError, match="no CPU path"):
        lm.next_logprobs([[2]])
    lm.to("cuda")
    rows = [[2], [2, 5], [2] + seqs[0]]
    got = lm.next_logprobs(rows).cpu().numpy()
    want = np.stack([ng.next_logprobs(m, r) for r in rows])
    assert np.abs(got - want).max() <= 1e-12  # the product's trainer is its own arithmetic; the bit-for-bit tests share one table
    hyps = [[2] + s + [2] for s in seqs[:5]]
    per = lm.token_logprobs(hyps)
    for x, p in zip(hyps, per):
        assert p.dtype == torch.float64 and p.shape[0] == len(x) - 1
        assert np.abs(p.numpy() - ng.token_logprobs(m, x)[1:]).max() <= 1e-12
    total = sum(float(p.sum()) for p in per)
    assert abs(lm.perplexity(seqs[:5]) - np.exp(-total / sum(len(x) - 1 for x in hyps))) <= 1e-9
    lm.to_arpa(tmp_path / "lm.arpa")
    back = P.NgramLM.from_arpa(tmp_path / "lm.arpa", fc.V_MODEL).to("cuda")
    assert np.abs(back.next_logprobs(rows).cpu().numpy() - got).max() <= 1e-12


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------------------
def test_create_refusals_name_the_gram_or_the_field(gu):
    lib = gu.lib()
    V = 5
    uni = [([w], -1.0, 0.0) for w in range(V)]

    def attempt(grams, order=3, vocab=V):
        lengths = [len(g[0]) for g in grams]
        symbols = np.zeros((len(grams), 8), np.int32)
        for i, g in enumerate(grams):
            symbols[i, :len(g[0])] = g[0]
        rc, h = create(gu, vocab, order, lengths, symbols, [g[1] for g in grams], [g[2] for g in grams])
        msg = lib.loco_last_error().decode() if rc else ""
        if rc == 0:
            lib.loco_ngram_destroy(h)
        return rc, msg

    assert attempt(uni + [([V], -99.0, -0.5), ([V, 3], -0.5, -0.1), ([V, 3, 4], -0.5, 0.0)]) == (0, "")  # <s> opens contexts
    cases = [(uni + [([3, 7], -1.0, 0.0)], "gram 5", "symbol 7"),
             (uni + [([3, -1], -1.0, 0.0)], "gram 5", "symbol -1"),
             (uni + [([3, V], -1.0, 0.0)], "gram 5", "predicted"),
             (uni + [([3, 4], -1.0, 0.0), ([3, V, 4], -1.0, 0.0)], "gram 6", "context"),
             (uni + [([3, 4], -1.0, 0.0), ([1, 2], -1.0, 0.0), ([3, 4], -2.0, 0.0)], "gram 7", "duplicate of gram 5"),
             (uni[:3] + uni[4:], "symbol 3", "unigram"),
             (uni + [([3, 4], float("nan"), 0.0)], "gram 5", "logp"),
             (uni + [([3, 4], -1.0, float("-inf"))], "gram 5", "backoff"),
             (uni + [([3, 4, 1, 2], -1.0, 0.0)], "gram 5", "length")]
    for grams, who, what in cases:
        rc, msg = attempt(grams)
        assert rc == -1 and who in msg and what in msg, (rc, msg)
    for kwargs, word in [(dict(order=9), "order"), (dict(order=0), "order"), (dict(vocab=128), "vocab"), (dict(vocab=0), "vocab")]:
        rc, msg = attempt(uni, **kwargs)
        assert rc == -1 and word in msg, (rc, msg)
    out = C.c_void_p()
    assert lib.loco_ngram_create(V, 3, 0, None, None, None, None, C.byref(out)) == -1 and "n = 0" in lib.loco_last_error().decode()
