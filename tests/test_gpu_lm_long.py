"""-m gpu: the GPT-2 scorer at GPT-2's own lengths -- n_positions = 1024, sequences of up to 1024 tokens, prefixes of up to 1023 -- against
HuggingFace in float64 (fixture lm4, tests/golden/make_lm_long_goldens.py; 2 layers, vocab 1003).

Uncached path (``token_nll``, ``token_nll_ragged``, ``model(...)``, ``nll_rows``): rows 64 .. 1023 of wpe, causal attention over 16 key
tiles, the two key splits the decoder attention takes at B = 1, S = 257 .. 341 (their premise is asserted, so a change of the split rule
turns the test red, not vacuous), a head of 1023 rows, and windows that start inside a longer token buffer at the real window length.

Cached path (``token_nll_given``, ``append``, ``score_carry``): a workgroup of lm_attention.hip owns 128 queries of one sequence, so
second .. eighth query tiles behind prefixes that end just before, at and just past a key tile, up to sixteen prefix tiles, P + L = 1024
and P = 1023.  The generator asserts that HuggingFace's cached and uncached float64 evaluations agree to 1e-12 at every cut used here, so
one set of NLLs serves both paths.

Bars are the suite's standing rule: an NLL may be 4 x what HuggingFace's own fp32 run, stored in the fixture, is away from float64; the
hidden states' relative L2 over the probe rows 4 x HuggingFace-fp32's and at most 2e-5.  tests/test_lm_long_ref.py shows on the CPU that a
one-key attention fault moves these NLLs by 100 x the bar and more."""
import importlib

import numpy as np
import pytest
import torch

from conftest import golden, record_figure

pytestmark = pytest.mark.gpu
la = importlib.import_module("loco-asr_amd")
lm = la.lm
_state = {}


def setup():
    if "m" not in _state:
        g = golden("lm4.npz")
        sd = la.synth.gpt2_state_dict(int(g["seed"]), int(g["n_layer"]), int(g["n_positions"]), int(g["vocab"]), float(g["logit_scale"]))
        _state["g"] = {k: g[k] for k in g.files}
        _state["m"] = la.GPT2LMHeadModelMI355X.from_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, n_positions=int(g["n_positions"])).to("cuda")
    return _state["g"], _state["m"]


def nll_bar(g):
    return 4.0 * float(g["hf_fp32_nll_max_abs_err"])


def cu(ids):
    return torch.from_numpy(np.asarray(ids, np.int64)).cuda()


def host(t):
    return t.double().cpu().numpy()


def bits(t):
    return t.contiguous().view(torch.int32)


def alone(k):
    """Sequence k of the fixture through token_nll with B = 1: computed once, shared by the tests that need it."""
    g, m = setup()
    if ("alone", k) not in _state:
        _state["alone", k] = host(m.token_nll(cu(g[f"ids{k}"])[None])[0])
    return _state["alone", k]


# ---- the uncached path --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 2, 3, 4])
def test_one_sequence_alone_against_hf_float64(k):
    g, m = setup()
    S = len(g[f"ids{k}"])
    assert S == (1024, 700, 341, 300, 257, 130)[k]
    nb = int(m._lib.loco_decoder_attention_scratch_bytes(1, S, S))
    if S in (341, 300, 257):
        assert nb > 0                                     # the premise: at B = 1 these lengths take key splits
    got = alone(k)
    assert got.shape == (S - 1,)
    err, bar = float(np.abs(got - g[f"nll{k}"]).max()), nll_bar(g)
    record_figure("lm_long_alone", fixture="lm4", S=S, split_bytes=nb, max_abs_err=err, bar=bar)
    print("lm4 alone", S, "split bytes", nb, "err", err, "bar", bar)
    assert err <= bar


def test_ragged_batch_against_hf_float64():
    """All six sequences in ONE right-padded call at S = 1024 with lengths 1024 .. 130.  The uncached path makes no bit-for-bit promise
    between a sequence alone and in a batch (the split count depends on B); their difference is recorded and held to the NLL bar."""
    g, m = setup()
    n_seq = int(g["n_seq"])
    got = m.token_nll_ragged([cu(g[f"ids{k}"]) for k in range(n_seq)], batch_size=8)
    got = [host(t) for t in got]
    assert [len(t) for t in got] == [len(g[f"ids{k}"]) - 1 for k in range(n_seq)]
    err = max(float(np.abs(t - g[f"nll{k}"]).max()) for k, t in enumerate(got))
    gap = max(float(np.abs(got[k] - alone(k)).max()) for k in range(n_seq))
    bar = nll_bar(g)
    record_figure("lm_long_ragged", fixture="lm4", sequences=n_seq, max_abs_err=err, alone_vs_batch_max_abs=gap, bar=bar)
    print("lm4 ragged err", err, "alone vs batch", gap, "bar", bar)
    assert err <= bar
    assert gap <= bar


def test_hidden_states_and_logits_at_1024():
    g, m = setup()
    ids, pos, probe = g["ids0"], g["probe_pos"], g["probe"]
    n_states = int(g["n_layer"]) + 1
    out = m(cu(ids)[None], output_hidden_states=True)
    assert len(out.hidden_states) == n_states and out.logits.shape == (1, 1024, int(g["vocab"]))
    rel = np.asarray([np.linalg.norm(host(out.hidden_states[i][0])[pos] - probe[i]) / np.linalg.norm(probe[i]) for i in range(n_states)])
    # the NLL recomputed in float64 from the returned logits, at the probe rows that have a next token
    rows = pos[pos < len(ids) - 1]
    z = host(out.logits[0])[rows]
    via_logits = np.log(np.exp(z - z.max(-1, keepdims=True)).sum(-1)) + z.max(-1) - z[np.arange(len(rows)), ids[rows + 1]]
    nll_err = float(np.abs(via_logits - g["nll0"][rows]).max())
    hf_rel, bar = float(g["hf_fp32_hidden_rel_l2"].max()), nll_bar(g)
    record_figure("lm_long_hidden", fixture="lm4", hidden_rel_l2=rel.tolist(), hidden_rel_l2_max=float(rel.max()), hf_fp32_hidden_rel_l2_max=hf_rel,
                  hidden_bar=min(4.0 * hf_rel, 2e-5), nll_via_logits_max_abs_err=nll_err, bar=bar)
    print("lm4 hidden rel l2", rel.tolist(), "(HF fp32:", g["hf_fp32_hidden_rel_l2"].tolist(), ") nll via logits", nll_err, "bar", bar)
    assert rel.max() <= 4.0 * hf_rel and rel.max() <= 2e-5
    assert nll_err <= bar


def test_max_len_windows_at_the_real_window_length():
    """The 1030-token recording at max_len = 1024: window 0 in full, then windows 1 .. 5 (one batch of 4 and one of 1, each a (start,
    length) pair into the recording's buffer) scored on their last position.  The targets are tokens 1 .. 1028: never the final one."""
    g, m = setup()
    rec, W = g["rec_ids"], int(g["max_len"])
    tokens = torch.from_numpy(rec.astype(np.int32)).cuda()
    got, targets, batches = [], [], 0
    for starts, first, last in lm.max_len_plan(len(rec), W, bsize=4):
        rows = np.arange(W - 1) if first else np.arange(len(starts)) * W + (W - 2)
        got.append(m.nll_rows(tokens, starts, [W] * len(starts), W, rows))
        targets += list(range(1, W)) if first else [o + W - 1 for o in starts]
        batches += 1
    assert targets == list(range(1, 1029)) and batches == 3
    got = host(torch.cat(got))
    err, bar = float(np.abs(got - g["rec_nll"]).max()), nll_bar(g)
    # the corpus walker scores the same rows
    tok = lm.TokenizedLines(eos_token_id=int(rec[-1]))
    nlls, ppl = lm.score_max_len(m, {"rec-A-0000-0100": " ".join(map(str, rec[:-1]))}, tok, bsize=4, max_len=W)
    walk_err = float(np.abs(np.asarray(nlls["rec"]) - g["rec_nll"]).max())
    record_figure("lm_long_max_len", fixture="lm4", windows=len(rec) - W, max_abs_err=err, walker_max_abs_err=walk_err, bar=bar)
    print("lm4 max_len err", err, "walker", walk_err, "bar", bar)
    assert err <= bar
    assert len(nlls["rec"]) == 1028 and walk_err <= bar
    assert abs(ppl["rec"] / float(np.exp(np.mean(np.asarray(nlls["rec"], np.float64)))) - 1.0) < 1e-12


def test_n_positions_is_accepted_and_one_more_is_refused_by_name():
    g, m = setup()
    assert m.n_positions == 1024 and alone(0).shape == (1023,)          # S = n_positions runs (and is checked above)
    ids = cu(np.concatenate([g["ids0"], g["ids1"][:1]]))
    assert ids.numel() == 1025
    with pytest.raises(ValueError, match="n_positions"):
        m.token_nll(ids[None])
    with pytest.raises(ValueError, match="n_positions"):
        m(ids[None])
    with pytest.raises(ValueError, match="n_positions"):
        m.nll_rows(ids.to(torch.int32), [0], [1025], 1025, [0])


# ---- the cached path ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,L", [(511, 1), (512, 129), (513, 200), (895, 129), (1023, 1), (512, 512)])
def test_token_nll_given_behind_a_long_prefix(P, L):
    """Sequence 0 (and, where P + L <= 700, sequence 1 on a second slot in the same call): second and fourth query tiles behind a prefix,
    prefixes that end one key short of, at and one key past a key tile, fourteen and sixteen prefix tiles, P + L = 1024."""
    g, m = setup()
    ks = [k for k in (0, 1) if P + L <= len(g[f"ids{k}"])]
    assert 0 in ks and ((P, L) not in ((1023, 1), (512, 512)) or P + L == m.n_positions)
    cache = m.new_cache(2)
    for k in ks:
        m.append(cache, k, cu(g[f"ids{k}"][:P]))
    got = m.token_nll_given(cache, [cu(g[f"ids{k}"][P:P + L]) for k in ks], slots=ks)
    assert [cache.length(k) for k in ks] == [P] * len(ks) and all(t.shape == (L,) for t in got)
    err = max(float(np.abs(host(t) - g[f"nll{k}"][P - 1:P - 1 + L]).max()) for k, t in zip(ks, got))
    bar = nll_bar(g)
    record_figure("lm_long_token_nll_given", fixture="lm4", P=P, L=L, sequences=len(ks), max_abs_err=err, bar=bar)
    print("lm4 given", P, L, ks, err, "bar", bar)
    assert err <= bar


def prefill():
    """append(score=True) of all 1024 tokens of sequence 0 on an empty slot (8 query tiles, 16 own key tiles): computed once."""
    g, m = setup()
    if "prefill" not in _state:
        cache = m.new_cache(1)
        _state["prefill"] = (cache, host(m.append(cache, 0, cu(g["ids0"]), score=True)))
    return _state["prefill"]


def test_prefill_of_1024_tokens_and_a_full_slot():
    g, m = setup()
    cache, got = prefill()
    assert got.shape == (1024,) and got[0] == 0.0
    err, bar = float(np.abs(got[1:] - g["nll0"]).max()), nll_bar(g)
    record_figure("lm_long_prefill", fixture="lm4", L=1024, max_abs_err=err, bar=bar)
    print("lm4 prefill", err, "bar", bar)
    assert err <= bar
    assert cache.length(0) == 1024
    with pytest.raises(ValueError, match=r"P \+ len = 1024 \+ 1 exceeds n_positions = 1024"):
        m.append(cache, 0, cu(g["ids1"][:1]))
    with pytest.raises(ValueError, match=r"P \+ len = 1024 \+ 1 exceeds n_positions = 1024"):
        m.token_nll_given(cache, [cu(g["ids1"][:1])], slots=0)
    assert cache.length(0) == 1024


def test_append_in_pieces_against_hf_float64():
    """300 + 424 tokens appended, then the last 300 scored behind them: another partition of the keys than the one-piece prefill, equal
    to it to rounding only; the difference is recorded."""
    g, m = setup()
    ids = g["ids0"]
    cache = m.new_cache(1)
    assert m.append(cache, 0, cu(ids[:300])) is None
    m.append(cache, 0, cu(ids[300:724]))
    assert cache.length(0) == 724
    got = host(m.append(cache, 0, cu(ids[724:]), score=True))
    assert cache.length(0) == 1024 and got.shape == (300,)
    err, bar = float(np.abs(got - g["nll0"][723:]).max()), nll_bar(g)
    gap = float(np.abs(got - prefill()[1][724:]).max())
    record_figure("lm_long_append_in_pieces", fixture="lm4", pieces=[300, 424, 300], max_abs_err=err, vs_one_piece_max_abs=gap, bar=bar)
    print("lm4 append in pieces", err, "vs one piece", gap, "bar", bar)
    assert err <= bar
    assert gap <= bar


def test_a_200_token_hypothesis_behind_513_keeps_its_bits():
    """The kernel's promise at these sizes: alone, among three others of 1, 129 and 64 tokens, on another slot that holds the same
    context, and twice in a row."""
    g, m = setup()
    P = 513
    cache = m.new_cache(3)
    m.append(cache, 0, cu(g["ids0"][:P]))
    m.append(cache, 1, cu(g["ids1"][:300]))               # another context between them
    m.append(cache, 2, cu(g["ids0"][:P]))
    hyp = cu(g["ids0"][P:P + 200])
    others = [cu(g["ids0"][P:P + 1]), cu(g["ids1"][:129]), cu(g["ids1"][129:193])]
    first = m.token_nll_given(cache, [hyp], slots=0)[0]
    err, bar = float(np.abs(host(first) - g["nll0"][P - 1:P + 199]).max()), nll_bar(g)
    assert err <= bar
    among = m.token_nll_given(cache, [others[0], hyp, others[1], others[2]], slots=0)[1]
    assert torch.equal(bits(among), bits(first))
    mixed = m.token_nll_given(cache, [others[1], others[2], hyp], slots=[1, 0, 2])[2]
    assert torch.equal(bits(mixed), bits(first))
    assert torch.equal(bits(m.token_nll_given(cache, [hyp], slots=2)[0]), bits(first))
    assert torch.equal(bits(m.token_nll_given(cache, [hyp], slots=0)[0]), bits(first))
    assert not torch.equal(m.token_nll_given(cache, [hyp], slots=1)[0], first)     # slot 1 holds another context
    assert [cache.length(s) for s in range(3)] == [P, 300, P]


class StreamTokenizer:
    """Makes ``lm.recordings`` rebuild a given id stream exactly: an utterance's text is its ids in decimal, the last of which is handed
    out as the <eos> that the walker appends after it (``eos_token_id`` is read right after the call)."""
    eos_token_id = None

    def __call__(self, text):
        ids = [int(t) for t in text.split()]
        self.eos_token_id = ids[-1]
        return {"input_ids": ids[:-1]}


CARRY_LENS = [200, 1, 129, 64, 300, 33, 129, 167, 1, 129, 129, 18]     # 1023 tokens, then 1 (P = 1023), then a rebase to P = 512


def utterances(rec, seq, lens):
    assert sum(lens) == len(seq)
    offs = np.concatenate([[0], np.cumsum(lens)])
    return {f"{rec}-A-{i:04d}00-{i:04d}99": " ".join(map(str, seq[a:b])) for i, (a, b) in enumerate(zip(offs[:-1], offs[1:]))}


def test_score_carry_with_1024_positions():
    """A recording of 1300 tokens (sequence 0, then the first 276 of sequence 1) in utterances of mixed lengths: the slot fills to
    exactly 1024, rebases to the last 512 tokens and goes on.  Alone (inflight = 1) and beside a second recording: the same NLLs.
    Against ``token_nll`` of each plan window on the GPU (the cached path against the uncached one) and, for the part of the first window
    that is sequence 0, against the fixture."""
    g, m = setup()
    seq = np.concatenate([g["ids0"], g["ids1"][:276]])
    assert len(seq) == 1300
    utts = utterances("recA", seq, CARRY_LENS)
    tok = StreamTokenizer()
    assert lm.recordings(utts, tok)["recA"] == seq.tolist()
    plan = list(lm.carry_plan(CARRY_LENS, m.n_positions))
    assert sum(p[4] for p in plan) >= 1 and (0, 1023, 1023, 1024, False) in plan and (512, 512, 1024, 1153, True) in plan
    one, ppl1 = lm.score_carry(m, utts, tok, inflight=1)
    both = dict(utts)
    both.update(utterances("recB", g["ids2"], [100, 1, 240]))
    two, ppl2 = lm.score_carry(m, both, tok, inflight=2)
    assert len(one["recA"]) == 1299 and len(two["recB"]) == 340
    assert two["recA"] == one["recA"] and ppl2["recA"] == ppl1["recA"]                # floats compared exactly: the same bits
    got = np.asarray(one["recA"])
    ref, windows = [], []
    for base in sorted({p[0] for p in plan}):
        chunks = [p for p in plan if p[0] == base]
        a, b = chunks[0][2], chunks[-1][3]
        w = host(m.token_nll(cu(seq[base:b])[None])[0])    # entry i scores stream token base + i + 1
        ref += list(w[max(a, 1) - base - 1:])
        windows.append((base, b))
    assert windows == [(0, 1024), (512, 1300)]
    bar = nll_bar(g)
    cross = float(np.abs(got - np.asarray(ref)).max())
    err = float(np.abs(got[:1023] - g["nll0"]).max())
    recb = float(np.abs(np.asarray(two["recB"]) - g["nll2"]).max())
    record_figure("lm_long_score_carry", fixture="lm4", chunks=len(plan), rebases=sum(p[4] for p in plan), cached_vs_uncached_max_abs=cross,
                  first_window_max_abs_err=err, second_recording_max_abs_err=recb, bar=bar)
    print("lm4 score_carry cached vs uncached", cross, "first window vs float64", err, "recB", recb, "bar", bar)
    assert cross <= bar
    assert err <= bar
    assert recb <= bar
