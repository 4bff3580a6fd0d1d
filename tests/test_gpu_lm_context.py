"""-m gpu: the GPT-2 scorer with a cached context -- ``token_nll_given`` / ``append`` / ``rescore`` / ``score_carry`` and the CLI's carry mode.

Against float64: the lm2 weights (12 layers, n_positions 64) with the numpy restatement ``lm_ref.token_nll`` on the concatenation context +
hypothesis, and the lm3 fixture (2 layers, n_positions 320: a prefix of several key tiles) with HuggingFace's float64 NLLs.  The bar is the
suite's standing rule: 4 x what HuggingFace's own fp32 run, stored in the same fixture, is away from float64.

Bit for bit: a hypothesis alone and among others, on permuted slots, scoring twice, ``append(score=True)`` against ``token_nll_given``, and a
recording walked alone or beside others.  A context built in two appends and the same context prefilled at once partition the keys
differently and agree only to rounding; the largest difference is recorded."""
import importlib
import json
import os
import pickle

import numpy as np
import pytest
import torch

import lm_ref
from conftest import golden, record_figure

pytestmark = pytest.mark.gpu
la = importlib.import_module("loco-asr_amd")
lm = la.lm
eval_ppl = importlib.import_module("loco-asr_amd.eval_ppl")
_models = {}


def model_of(name):
    if name not in _models:
        g = golden(name + ".npz")
        sd = la.synth.gpt2_state_dict(int(g["seed"]), int(g["n_layer"]), int(g["n_positions"]), int(g["vocab"]), float(g["logit_scale"]))
        m = la.GPT2LMHeadModelMI355X.from_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, n_positions=int(g["n_positions"])).to("cuda")
        _models[name] = (g, sd, m)
    return _models[name]


def cu(ids):
    return torch.from_numpy(np.asarray(ids, np.int64)).cuda()


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return len(a) == len(b) and all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("L", [1, 2, 31])
@pytest.mark.parametrize("P", [1, 31, 32, 33])
def test_token_nll_given_against_the_float64_restatement(P, L):
    """lm2: two hypotheses of L tokens behind a context of P (P + L <= 64, with equality at 33 + 31), one the fixture sequence's own
    continuation, one taken from another sequence."""
    g, sd, m = model_of("lm2")
    stream, other = g["ids5"], g["ids4"]
    assert P + L <= 64
    hyps = [stream[P:P + L], other[:L] if L <= len(other) else np.concatenate([other, g["ids0"]])[:L]]
    cache = m.new_cache(1)
    m.append(cache, 0, cu(stream[:P]))
    got = m.token_nll_given(cache, [cu(h) for h in hyps], slots=0)
    assert cache.length(0) == P
    err = 0.0
    for h, t in zip(hyps, got):
        ref = lm_ref.token_nll(sd, np.concatenate([stream[:P], h]))[P - 1:]
        assert t.shape == (L,)
        err = max(err, float(np.abs(t.double().cpu().numpy() - ref).max()))
    bar = 4.0 * float(g["hf_fp32_nll_max_abs_err"])
    record_figure("lm_token_nll_given", fixture="lm2", P=P, L=L, max_abs_err=err, bar=bar)
    print("lm2 given", P, L, err, "bar", bar)
    assert err <= bar


@pytest.mark.parametrize("L", [1, 33, 63])
@pytest.mark.parametrize("P", [63, 64, 65, 257])
def test_token_nll_given_against_hf_float64_on_a_long_prefix(P, L):
    """lm3: the prefix ends one key short of, at, and one key past a key tile, and deep into the fifth; 257 + 63 fills n_positions = 320
    exactly.  Sequences 0 and 1 of the fixture go through one call on two slots where both are long enough."""
    g, _, m = model_of("lm3")
    ks = [k for k in (0, 1) if P + L <= len(g[f"ids{k}"])]
    assert ks and ((P, L) != (257, 63) or P + L == int(g["n_positions"]))
    cache = m.new_cache(2)
    for k in ks:
        m.append(cache, k, cu(g[f"ids{k}"][:P]))
    got = m.token_nll_given(cache, [cu(g[f"ids{k}"][P:P + L]) for k in ks], slots=ks)
    err = max(float(np.abs(t.double().cpu().numpy() - g[f"nll{k}"][P - 1:P - 1 + L]).max()) for k, t in zip(ks, got))
    bar = 4.0 * float(g["hf_fp32_nll_max_abs_err"])
    record_figure("lm_token_nll_given", fixture="lm3", P=P, L=L, sequences=len(ks), max_abs_err=err, bar=bar)
    print("lm3 given", P, L, ks, err, "bar", bar)
    assert err <= bar


def test_a_hypothesis_does_not_depend_on_its_neighbours_or_its_slot():
    g, _, m = model_of("lm2")
    ctx = g["ids5"][:20]
    cache = m.new_cache(3)
    m.append(cache, 0, cu(ctx))
    m.append(cache, 2, cu(ctx))                             # the same context on another slot
    m.append(cache, 1, cu(g["ids4"][:7]))                   # and a different one between them
    hyps = [cu(g["ids5"][20:20 + n]) for n in (9, 1, 33)] + [cu(g["ids4"][:17]), cu(g["ids0"][:2])]
    among = m.token_nll_given(cache, hyps, slots=0)
    for n, h in enumerate(hyps):
        assert same_bits(m.token_nll_given(cache, [h], slots=0), [among[n]]), n
    assert same_bits(m.token_nll_given(cache, hyps, slots=[0, 2, 0, 2, 2]), among)
    order = [3, 0, 4, 2, 1]
    moved = m.token_nll_given(cache, [hyps[i] for i in order] + [hyps[0]], slots=[2, 0, 0, 2, 0, 1])
    assert same_bits(moved[:5], [among[i] for i in order])
    assert not torch.equal(moved[5], among[0])              # slot 1 holds another context
    # the cache is unchanged: lengths, and a second identical call
    assert [cache.length(s) for s in range(3)] == [20, 7, 20]
    assert same_bits(m.token_nll_given(cache, hyps, slots=0), among)
    nlls, totals = lm.rescore(m, cu(ctx), hyps)
    assert same_bits(nlls, among)
    assert totals.dtype == torch.float64 and np.allclose(totals.cpu().numpy(), [float(t.double().sum()) for t in among], rtol=1e-15)


def test_append_in_pieces_and_append_with_score():
    g, _, m = model_of("lm2")
    ids = g["ids5"]
    cache = m.new_cache(2)
    assert m.append(cache, 0, cu(ids[:10])) is None
    m.append(cache, 0, cu(ids[10:20]))
    m.append(cache, 1, cu(ids[:20]))
    assert (cache.length(0), cache.length(1)) == (20, 20)
    hyp = cu(ids[20:53])
    a, b = m.token_nll_given(cache, [hyp, hyp], slots=[0, 1])
    gap = float((a.double() - b.double()).abs().max())
    bar = 4.0 * float(g["hf_fp32_nll_max_abs_err"])
    record_figure("lm_append_in_pieces", max_abs_diff=gap, bar=bar, bit_equal=bool(torch.equal(a, b)))
    print("append in pieces vs at once", gap, "bar", bar)
    assert gap <= bar
    # append(score=True) is token_nll_given of the same ids, bit for bit, and extends the slot
    scored = m.append(cache, 1, hyp, score=True)
    assert torch.equal(bits(scored), bits(b)) and cache.length(1) == 53
    # on an empty slot the first token scores 0 and the rest is the plain causal model
    cache.reset(0)
    assert cache.length(0) == 0
    first = m.append(cache, 0, cu(ids[:17]), score=True)
    plain = m.token_nll(cu(ids[:17])[None])[0]
    assert float(first[0]) == 0.0 and float((first[1:].double() - plain.double()).abs().max()) <= bar


def carry_corpus(V):
    """Recording recA: 150 tokens in utterances of 1, 2, 31, 32, 33, 20 and 31 tokens (<eos> included: the first is an empty line);
    recB and recC walk beside it."""
    utts, lens = {}, {"recA": [1, 2, 31, 32, 33, 20, 31], "recB": [5, 30, 5], "recC": [40, 9, 40, 9]}
    for rec, ls in lens.items():
        for i, n in enumerate(ls):
            ids = la.synth.gpt2_token_ids(n - 1, V - 1, f"carry/{rec}/{i}") if n > 1 else []
            utts[f"{rec}-A-{i:04d}00-{i:04d}99"] = " ".join(map(str, ids))
    return utts, lens


def test_score_carry_against_its_plan_windows_and_beside_other_recordings():
    g, sd, m = model_of("lm2")
    V, keep = int(g["vocab"]), 16
    utts, lens = carry_corpus(V)
    tok = lm.TokenizedLines(eos_token_id=V - 1)
    seq = np.asarray(lm.recordings(utts, tok)["recA"])
    assert len(seq) == 150
    nlls3, ppl3 = lm.score_carry(m, utts, tok, keep=keep, inflight=3)
    nlls1, ppl1 = lm.score_carry(m, utts, tok, keep=keep, inflight=1)
    alone, _ = lm.score_carry(m, {u: t for u, t in utts.items() if u.startswith("recA")}, tok, keep=keep, inflight=2)
    assert {r: len(v) for r, v in nlls3.items()} == {r: sum(ls) - 1 for r, ls in lens.items()}
    assert nlls1 == nlls3 and ppl1 == ppl3 and alone["recA"] == nlls3["recA"]          # floats compared exactly: the same bits
    plan = list(lm.carry_plan(lens["recA"], 64, keep))
    assert sum(p[4] for p in plan) >= 2
    ref = []
    for base, P, a, b, _ in plan:
        w = lm_ref.token_nll(sd, seq[base:b])              # entry i scores stream token base + i + 1
        ref += list(w[max(a, 1) - base - 1:])
    err = float(np.abs(np.asarray(nlls3["recA"]) - np.asarray(ref)).max())
    bar = 4.0 * float(g["hf_fp32_nll_max_abs_err"])
    record_figure("lm_score_carry", max_abs_err=err, bar=bar, chunks=len(plan), rebases=sum(p[4] for p in plan))
    print("score_carry", err, "bar", bar)
    assert err <= bar
    for r, v in nlls3.items():
        assert abs(ppl3[r] / float(np.exp(np.mean(np.asarray(v, np.float64)))) - 1.0) < 1e-12


def test_cli_carry_mode_writes_the_two_files(tmp_path):
    V = 1003
    lines, want = [], {}
    for i in range(30):
        rec, n = f"rec{i % 3}", 2 + (i * 7) % 9
        ids = la.synth.gpt2_token_ids(n, V - 1, f"cli/{i}")
        lines.append(f"{rec}-A-{i:04d}00-{i:04d}99 " + " ".join(map(str, ids)))
        want[rec] = want.get(rec, 0) + n + 1
    src = tmp_path / "fisher.txt"
    src.write_text("\n".join(lines[::-1]) + "\n")
    out = tmp_path / "carry"
    assert eval_ppl.main(["--in_file", str(src), "--random-init", "--layers", "2", "--positions", "32", "--vocab", str(V), "--tokenized",
                          "--out_dir", str(out), "--context_type", "carry", "--keep", "8"]) == 0
    with open(out / "rec_id2nlls.pkl", "rb") as fh:
        nlls = pickle.load(fh)
    with open(out / "rec_id2ppl.json") as fh:
        ppl = json.load(fh)
    assert set(nlls) == set(ppl) == {"rec0", "rec1", "rec2"}
    for r in nlls:                                          # every token of the recording but its very first
        assert len(nlls[r]) == want[r] - 1 and all(np.isfinite(nlls[r])), r
        assert abs(ppl[r] / float(np.exp(np.mean(nlls[r]))) - 1.0) < 1e-9
    log = [f for f in os.listdir(out) if f.endswith(".log")]
    assert log == ["gpt2_carry_fisher.log"] and "Avg. PPL of recordings:" in (out / log[0]).read_text()


def test_named_errors():
    """Host-side checks and the status word; nothing here reaches a kernel with a bad shape."""
    g, _, m = model_of("lm2")
    ids = g["ids5"]
    cache = m.new_cache(2)
    m.append(cache, 0, cu(ids[:60]))
    with pytest.raises(ValueError, match=r"P \+ len = 60 \+ 5 exceeds n_positions = 64"):
        m.token_nll_given(cache, [cu(ids[:5])], slots=0)
    with pytest.raises(ValueError, match="exceed n_positions"):
        lm.rescore(m, cu(ids[:60]), [cu(ids[:5])])
    tokens = cu(ids[:8]).to(torch.int32)
    with pytest.raises(ValueError, match="two committing sequences on slot 1"):
        m._ctx_step(cache, tokens, [(0, 2, 1, lm.CTX_COMMIT), (2, 2, 1, lm.CTX_COMMIT | lm.CTX_SCORE)])
    with pytest.raises(ValueError, match="slot = 2 is outside 0 .. 1"):
        m.token_nll_given(cache, [cu(ids[:2])], slots=2)
    with pytest.raises(ValueError, match="at least one"):
        m.token_nll_given(cache, [cu(ids[:0])], slots=1)
    assert (cache.length(0), cache.length(1)) == (60, 0)    # a refused call changes nothing
    bad = ids[:4].copy()
    bad[1] = int(g["vocab"])
    with pytest.raises(ValueError, match=r"position 4 .*outside \[0, 1003\)"):
        m.token_nll_given(cache, [cu(ids[:3]), cu(bad)], slots=1)
    with pytest.raises(ValueError, match="outside 1 .. 64"):
        m.new_cache(65)
