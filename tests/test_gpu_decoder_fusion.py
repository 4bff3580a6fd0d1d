"""Shallow fusion of an n-gram model into the beam search of the decoder slot pool, on the GPU (csrc/ngram.hip, csrc/decoder_beam.hip).

1. loco_op_beam_select_fused against tests/decoder_fusion_ref.py, exact in every array; a step in which the bonus changes the candidate
   order, a tie that only the flat index resolves; bonus = NULL equals loco_op_beam_select.
2. The model of tests/test_gpu_decoder_beam.py (2 + 2 layers) with fusion_cases.fusion_model at weight 1, bonus 0.3:
   ``beam_search_many(lm=...)`` replayed through the restatement with the bonus of tests/ngram_ref.py on the restatement's own token
   rows -- hypotheses, scores and sums the same bits; the fused lists differ from the plain ones and hold several lengths.
3. Invariance: the same bits at slots = K, 2K and 64, in reversed admission order and beside a 30 s clip; both weights 0 give the plain
   search; greedy ``generate_many`` on the same handle is unchanged.
4. Identity: sequence_logprobs = sum(token_logprobs) + w * lm_logprobs + b * (len - 1) within 2^-52 * n * sum|terms|.
5. ``transcribe_long`` takes the model; the command line writes "lm_logprob"; refusals by name.
"""
import ctypes as C
import importlib
import json
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import decoder_beam_ref as ref
import decoder_fusion_ref as fref
import fusion_cases as fc
import ngram_ref as ng
from test_gpu_decoder_beam import (CAPS, CLIPS, K_MODEL, Guarded, beam_config, beam_model, beams, clips_of, den_host, same_bits, select_op)
from test_gpu_decoder_pool import batches_of
from test_gpu_decoder_score import GAP

pytestmark = pytest.mark.gpu

W, B = fc.LM_WEIGHT, fc.LM_BONUS
_cache = {}


@pytest.fixture(scope="module")
def gu():
    return importlib.import_module("gpu_util")


def select_fused(gu, groups, logits, ld, cfg, den, bonus):
    """One loco_op_beam_select_fused step on the state of ``groups``: ({array name: host array}, logprobs, poll)."""
    G, K, V, S = len(groups), groups[0].K, groups[0].V, groups[0].S
    cat = lambda name: np.concatenate([getattr(g, name) for g in groups])  # noqa: E731
    st = {n: Guarded(cat(n)) for n in ref.BeamGroup.ARRAYS if n not in ("parent", "count")}
    st["parent"] = Guarded(np.full(G * K, -77, np.int32))
    st["count"] = Guarded(np.full(G * K, -77, np.int32))
    x = Guarded(np.asarray(logits, np.float32))
    lp = Guarded(np.full((G * K, V), 123.0, np.float32))
    pl = Guarded(np.full(1, -7, np.int32))
    d = Guarded(den)
    bn = Guarded(np.asarray(bonus, np.float64)) if bonus is not None else None
    gu.check(gu.lib().loco_op_beam_select_fused(
        x.ptr, ld, G, V, S, C.byref(cfg), d.ptr, st["status"].ptr, st["pos"].ptr, st["caps"].ptr, st["cur"].ptr, st["cnt"].ptr, st["lengths"].ptr,
        st["tokens"].ptr, st["tlp"].ptr, st["run"].ptr, st["alive"].ptr, st["unsat"].ptr, st["fin_n"].ptr, st["fin_score"].ptr, st["fin_sum"].ptr,
        st["fin_len"].ptr, st["fin_tok"].ptr, st["fin_tlp"].ptr, lp.ptr, st["parent"].ptr, st["count"].ptr, pl.ptr, bn.ptr if bn else None,
        gu.stream()), "loco_op_beam_select_fused")
    torch.cuda.synchronize()
    if bn is not None:
        assert same_bits(bn.back(), np.asarray(bonus, np.float64))  # only read
    return {n: v.back() for n, v in st.items()}, lp.back(), int(pl.back()[0])


def fused_step_and_compare(gu, groups, rows, bonus, cfg, den, pad=5):
    """One step of the operator and of the restatement (on the operator's log-probabilities, with the same bonus): every array agrees."""
    G, K, V = len(groups), groups[0].K, groups[0].V
    x = np.full((G * K, V + pad), GAP, np.float32)
    x[:, :V] = rows
    was_open = [g.open for g in groups]
    got, lp, poll = select_fused(gu, groups, x, V + pad, cfg, den, bonus)
    for i, g in enumerate(groups):
        g.step(lp[i * K:(i + 1) * K], None if bonus is None else bonus[i * K:(i + 1) * K])
    for n in ref.BeamGroup.ARRAYS:
        want = np.concatenate([getattr(g, n) + (i * K if n == "parent" else 0) for i, g in enumerate(groups)])
        if n in ("parent", "count"):
            want = np.where(np.repeat([not o for o in was_open], K), -77, want)
        assert same_bits(got[n], want.astype(got[n].dtype)), (n, got[n], want)
    assert poll == sum(int(g.open) * K for g in groups)
    return lp


# ---- 1. the select operator ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,K", [(81, 1), (81, 3), (81, 4), (32, 16), (127, 5)])
def test_fused_select_matches_the_restatement(gu, V, K):
    S = 9
    rng = np.random.default_rng(100 * V + K)
    for n, G in enumerate(sorted({1, 3, 64 // K})):
        length_penalty, early = [(1.0, False), (0.0, True), (2.0, "never")][(n + K) % 3]
        cfg, den = beam_config(gu, K, length_penalty, early), den_host(gu, length_penalty, S)
        groups = [fref.FusedBeamGroup(K, V, S, cap=4 + (g % 5), length_penalty=length_penalty, early_stopping=early, den=den) for g in range(G)]
        plain = [fref.FusedBeamGroup(K, V, S, cap=4 + (g % 5), length_penalty=length_penalty, early_stopping=early, den=den) for g in range(G)]
        reordered = False
        for j in range(8):
            rows = (rng.standard_normal((G * K, V)) * 2.0).astype(np.float32)
            rows[:, ref.EOS] += (-60.0 if j == 0 else rng.uniform(-2.0, 5.0))
            bonus = rng.standard_normal((G * K, V)) * 2.0 + 0.3
            lp = fused_step_and_compare(gu, groups, rows, bonus, cfg, den)
            if j == 0:  # the same first step without the bonus takes other candidates
                for i, (g, p) in enumerate(zip(groups, plain)):
                    p.step(lp[i * K:(i + 1) * K])
                    reordered |= g.tokens[:, 1].tolist() != p.tokens[:, 1].tolist()
            for g in groups:
                g.reorder()
        assert reordered  # in the first step the bonus changed which candidates were taken
        assert not any(g.open for g in groups)


def test_fused_ties_go_to_the_lower_flat_index(gu):
    """Three equal rows with the same bonus: candidates (k, 11) and (k, 20) of every beam tie in the fused score, bit for bit, and
    only the flat index k V + v orders them; a column the bonus pushes down stays out."""
    K, V, S = 3, 32, 6
    cfg, den = beam_config(gu, K), den_host(gu, 1.0, S)
    g = fref.FusedBeamGroup(K, V, S, cap=6, den=den)
    g.alive[:], g.run[:], g.pos[:] = 1, -1.5, 1
    g.tokens[:, 1], g.cur[:], g.cnt[:] = [7, 8, 9], [7, 8, 9], 2
    row = np.zeros(V, np.float32)
    row[[11, 20]] = [3.0, 3.0]
    bonus = np.zeros((K, V))
    bonus[:, [11, 20]] = 0.25
    bonus[:, 5] = -4.0
    fused_step_and_compare(gu, [g], np.tile(row, (K, 1)), bonus, cfg, den)
    assert g.parent.tolist() == [0, 0, 1] and g.tokens[:, 2].tolist() == [11, 20, 11] and g.run[0] == g.run[1] == g.run[2]


def test_null_bonus_is_the_plain_operator(gu):
    K, V, S = 4, 81, 8
    cfg, den = beam_config(gu, K), den_host(gu, 1.0, S)
    rng = np.random.default_rng(4)
    a = [ref.BeamGroup(K, V, S, cap=5 + g, den=den) for g in range(3)]
    for j in range(5):
        rows = (rng.standard_normal((3 * K, V)) * 3.0).astype(np.float32)
        rows[:, ref.EOS] += -60.0 if j == 0 else 2.0
        x = np.full((3 * K, V + 7), GAP, np.float32)
        x[:, :V] = rows
        plain, lp_a, poll_a = select_op(gu, a, x, V + 7, cfg, den)
        fused, lp_b, poll_b = select_fused(gu, a, x, V + 7, cfg, den, None)
        assert poll_a == poll_b and same_bits(lp_a, lp_b)
        for n in plain:
            assert same_bits(plain[n], fused[n]), n
        for i, g in enumerate(a):
            g.step(lp_a[i * K:(i + 1) * K])
            g.reorder()


# ---- 2. the model ------------------------------------------------------------------------------------------------------------------------
def fusion_lm(gu):
    """(the restatement's model, the product's NgramLM over the same table, on the device)."""
    if "lm" not in _cache:
        P = importlib.import_module("loco-asr_amd.ngram")
        m = fc.fusion_model()
        _cache["lm"] = (m, P.NgramLM(m.order, m.V, *ng.arrays(m)).to("cuda"))
    return _cache["lm"]


@pytest.fixture(scope="module")
def fused(gu):
    return beams(gu, return_step_logprobs=True, lm=fusion_lm(gu)[1], lm_weight=W, lm_bonus=B)


@pytest.fixture(scope="module")
def plain(gu):
    return beams(gu)


def test_fused_search_replays_through_the_restatement(gu, fused, plain):
    hyps, scores = fused
    m, _ = fusion_lm(gu)
    V = beam_model(gu).speecht5.encoder._decoder_vocab
    assert V == fc.V_MODEL
    lengths, differ = set(), 0
    for u in range(CLIPS):
        g = fref.FusedBeamGroup(K_MODEL, V, max(CAPS), CAPS[u])
        for lp in hyps.step_logprobs[u].numpy():
            assert g.open and g.step(lp, fref.fused_bonus(fref.lm_rows(ng, m, g), W, B))
            g.reorder()
        assert not g.open
        want = g.finished()
        assert len(want) == len(hyps[u]) == K_MODEL
        for h, (tok, score, total, tlp) in enumerate(want):
            assert hyps[u][h].tolist() == tok, (u, h)
            assert same_bits(np.float64(hyps.sequence_scores[u][h].item()), np.float64(score))
            assert same_bits(np.float64(hyps.sequence_logprobs[u][h].item()), np.float64(total))
            assert same_bits(scores[u][h].numpy(), tlp[1:])
            lengths.add(len(tok))
        differ += [h.tolist() for h in hyps[u]] != [h.tolist() for h in plain[0][u]]
    assert differ >= 1 and len(lengths) >= 2, (differ, lengths)  # a real change, and not the trivial regime


def test_fused_search_replays_at_a_weight_whose_product_rounds(gu):
    """At weight 1 the product weight * lm is exact, and a fused multiply-add gives what a product and a sum give.  At 0.7 it is
    not: the device's bonus must still be the restatement's two roundings, or run, the sums and the order drift by an ulp."""
    w, b = 0.7, 0.3
    m, lm = fusion_lm(gu)
    hyps, scores = beams(gu, return_step_logprobs=True, lm=lm, lm_weight=w, lm_bonus=b)
    inexact = 0
    for u in range(CLIPS):
        g = fref.FusedBeamGroup(K_MODEL, fc.V_MODEL, max(CAPS), CAPS[u])
        for lp in hyps.step_logprobs[u].numpy():
            rows = fref.lm_rows(ng, m, g)
            bonus = fref.fused_bonus(rows, w, b)
            once = np.array([[float(Fraction(w) * Fraction(float(x)) + Fraction(b)) for x in r] for r in rows])  # one rounding: an FMA
            inexact += int((once != bonus).sum())
            assert g.open and g.step(lp, bonus)
            g.reorder()
        want = g.finished()
        assert len(want) == len(hyps[u]) == K_MODEL
        for h, (tok, score, total, tlp) in enumerate(want):
            assert hyps[u][h].tolist() == tok, (u, h)
            assert same_bits(np.float64(hyps.sequence_scores[u][h].item()), np.float64(score))
            assert same_bits(np.float64(hyps.sequence_logprobs[u][h].item()), np.float64(total))
            assert same_bits(scores[u][h].numpy(), tlp[1:])
    assert inexact > 0  # some bonus of the replay differs between one rounding and two


# ---- 3. invariance ---------------------------------------------------------------------------------------------------------------------
def decode_fused(gu, items, slots, T_cap, S_max, weight=W, bonus=B):
    dec = importlib.import_module("loco-asr_amd.decoder")
    cfg = dec.check_beam_args(K_MODEL, K_MODEL)[2]
    pool = dec.DecoderPool(beam_model(gu).speecht5.encoder, slots, T_cap, S_max, torch.device("cuda", 0), beam=cfg,
                           fusion=(fusion_lm(gu)[1], weight, bonus))
    pool.submit(list(items))
    return {k: rest for k, *rest in pool.drain()}


def test_fused_result_does_not_depend_on_slots_order_or_neighbours(gu, fused):
    from test_gpu_decoder_pool import encode
    clips = clips_of(gu) + [(4, 480000)]
    items, out, _ = encode(gu, beam_model(gu), clips, CAPS + [5])
    T_cap, S_max = max(it.rows for it in items), max(CAPS)
    base = decode_fused(gu, items, 64, T_cap, S_max)
    assert sorted(base) == list(range(CLIPS + 1))
    for slots, chosen in [(K_MODEL, items[:CLIPS]), (2 * K_MODEL, list(reversed(items))), (64, list(reversed(items[:CLIPS])))]:
        got = decode_fused(gu, chosen, slots, T_cap, S_max)
        assert sorted(got) == sorted(it.key for it in chosen)
        for k, (hyps, scores, sums, tlps, _) in got.items():
            want = base[k]
            assert len(hyps) == len(want[0])
            for h in range(len(hyps)):
                assert torch.equal(hyps[h], want[0][h]) and same_bits(tlps[h].numpy(), want[3][h].numpy()), (slots, k, h)
            assert same_bits(scores.numpy(), want[1].numpy()) and same_bits(sums.numpy(), want[2].numpy()), (slots, k)


def test_zero_weights_are_the_plain_search_and_greedy_is_untouched(gu, fused, plain):
    model = beam_model(gu)
    batches = batches_of(gu, clips_of(gu))
    before, before_scores = model.generate_many(batches, max_length=CAPS, return_scores=True)
    zero, zero_scores = beams(gu, lm=fusion_lm(gu)[1], lm_weight=0.0, lm_bonus=0.0)
    hyps, scores = plain
    for u in range(CLIPS):
        assert [h.tolist() for h in zero[u]] == [h.tolist() for h in hyps[u]], u
        assert bool((zero.sequence_scores[u] == hyps.sequence_scores[u]).all()) and bool((zero.sequence_logprobs[u] == hyps.sequence_logprobs[u]).all())
        assert all(same_bits(a.numpy(), b.numpy()) for a, b in zip(zero_scores[u], scores[u]))
        assert zero.lm_logprobs[u].shape == (K_MODEL,) and hyps.lm_logprobs is None
    after, after_scores = model.generate_many(batches, max_length=CAPS, return_scores=True)
    for u in range(CLIPS):
        assert torch.equal(before[u], after[u]) and same_bits(before_scores[u].cpu().numpy(), after_scores[u].cpu().numpy())


# ---- 4. identity -------------------------------------------------------------------------------------------------------------------------
def test_fused_sum_is_acoustic_plus_weighted_lm_plus_bonus(gu, fused):
    hyps, scores = fused
    m, _ = fusion_lm(gu)
    for u in range(CLIPS):
        for h in range(K_MODEL):
            ids, tlp = hyps[u][h].tolist(), scores[u][h].double().numpy()
            lm = float(hyps.lm_logprobs[u][h])
            assert abs(lm - float(ng.token_logprobs(m, ids).sum())) <= 2.0 ** -52 * len(ids) * abs(lm)  # loco_op_ngram_score's tokens, summed
            n = 3 * (len(ids) - 1)  # per generated token: its log P, w * its n-gram log P, b
            terms = float(np.abs(tlp).sum()) + abs(W) * abs(lm) + abs(B) * (len(ids) - 1)
            want = math.fsum(tlp.tolist()) + W * lm + B * (len(ids) - 1)
            got = float(hyps.sequence_logprobs[u][h])
            assert abs(got - want) <= 2.0 ** -52 * n * terms, (u, h, got, want)
            assert float(hyps.sequence_scores[u][h]) == got / float(len(ids) - 1) ** 1.0


# ---- 5. pass-through, command line, refusals ----------------------------------------------------------------------------------------------
def test_transcribe_long_takes_the_model(gu, fused):
    from segment_cases import LONG, recording
    model, (_, lm) = beam_model(gu), fusion_lm(gu)
    wave = gu.dev(recording())
    four = model.transcribe_long(wave, vad=LONG, max_length=12, return_scores=True, num_beams=4, lm=lm, lm_weight=W, lm_bonus=B)
    assert len(four.segments) >= 2
    for c in four.segments:
        clip = wave[round(c.start_s * 16000):round(c.end_s * 16000)][None]
        best = model.beam_search_many([dict(input_values=clip, attention_mask=torch.ones_like(clip, dtype=torch.int32))], num_beams=4, max_length=12,
                                      lm=lm, lm_weight=W, lm_bonus=B)
        assert torch.equal(best[0][0], c.ids) and c.token_logprobs.shape[0] == c.ids.shape[0] - 1
    with pytest.raises(ValueError, match="num_beams"):
        model.transcribe_long(wave, vad=LONG, lm=lm, lm_weight=W)


def test_refusals_by_name(gu, fused):
    P = importlib.import_module("loco-asr_amd.ngram")
    dec = importlib.import_module("loco-asr_amd.decoder")
    model, (_, lm) = beam_model(gu), fusion_lm(gu)
    batches = batches_of(gu, clips_of(gu)[:2])
    small = P.NgramLM.train([[4, 5, 6]], 2, 30).to("cuda")
    with pytest.raises(ValueError, match="vocab"):
        model.beam_search_many(batches, num_beams=4, lm=small, lm_weight=1.0)
    with pytest.raises(ValueError, match="lm_weight"):
        model.beam_search_many(batches, num_beams=4, lm=lm, lm_weight=float("nan"))
    with pytest.raises(ValueError, match="lm_bonus"):
        model.beam_search_many(batches, num_beams=4, lm=lm, lm_weight=1.0, lm_bonus=float("inf"))
    # the C entry point: another vocabulary, a weight that is not finite, a pool that has admitted groups
    enc, lib = model.speecht5.encoder, gu.lib()
    cfg = dec.check_beam_args(2)[2]
    pool = dec.DecoderPool(enc, 4, 8, 6, torch.device("cuda", 0), beam=cfg, fusion=(lm, W, B))
    ws = pool.workspace
    attach = lambda h, w: lib.loco_decoder_pool_attach_ngram(enc._handle, 4, 8, 6, h, w, 0.0, gu.ptr(ws), ws.numel())  # noqa: E731
    assert attach(lm.handle, 1.0) == -2 and "attached" in lib.loco_last_error().decode()
    fresh = dec.DecoderPool(enc, 4, 8, 6, torch.device("cuda", 0), beam=cfg)
    fws = torch.empty(int(lib.loco_decoder_beam_fusion_workspace_bytes(enc._handle, 4, 8, 6, 2)), dtype=torch.uint8, device="cuda")
    assert fws.numel() > fresh.workspace.numel() == int(lib.loco_decoder_beam_workspace_bytes(enc._handle, 4, 8, 6, 2))
    gu.check(lib.loco_decoder_pool_init(enc._handle, 4, 8, 6, gu.ptr(fws), fws.numel(), gu.stream()), "loco_decoder_pool_init")
    at = lambda h, w, t=fws: lib.loco_decoder_pool_attach_ngram(enc._handle, 4, 8, 6, h, w, 0.0, gu.ptr(t), t.numel())  # noqa: E731
    assert at(small.handle, 1.0) == -1 and "vocab" in lib.loco_last_error().decode()
    assert at(lm.handle, float("inf")) == -1 and "weight" in lib.loco_last_error().decode()
    assert at(lm.handle, 1.0, fresh.workspace) == -3 and "loco_decoder_beam_fusion_workspace_bytes" in lib.loco_last_error().decode()
    assert at(lm.handle, 1.0) == 0
    out = torch.zeros((2, 8, 768), device="cuda")
    frames = torch.tensor([8, 8], dtype=torch.int32, device="cuda")
    pool.submit([dec.PoolItem(key=i, enc_out=out, frames=frames, clip=i, rows=8, cap=4) for i in range(2)])
    assert len(pool.drain()) == 2  # the pool with the model attached runs to its end


def test_command_line_writes_lm_logprob(gu, fused, tmp_path, monkeypatch):
    tr = importlib.import_module("loco-asr_amd.transcribe")
    fe = importlib.import_module("loco-asr_amd.feature_extractor")
    P = importlib.import_module("loco-asr_amd.ngram")
    model = beam_model(gu)
    monkeypatch.setattr(tr, "build_model", lambda args: model)
    arpa = tmp_path / "lm.arpa"
    fusion_lm(gu)[1].to_arpa(arpa)
    lm = P.NgramLM.from_arpa(arpa, fc.V_MODEL)
    common = ["--random-init", "--synthetic", "4", "--synthetic-seconds", "1.5", "--slots", "16", "--max-length", "12"]

    def run(extra):
        out = tmp_path / "out.jsonl"
        assert tr.main(common + extra + ["--out", str(out)]) == 0
        return [json.loads(l) for l in out.read_text().splitlines()]

    items = tr.gather_items(tr.build_parser().parse_args(common))
    processor = fe.SpeechT5FeatureExtractorMI355X()
    feats = [tr.load_batch(items[b0:b0 + 2], b0, processor, torch.device("cuda", 0)) for b0 in (0, 2)]
    want = model.beam_search_many(feats, num_beams=4, num_return_sequences=3, max_length=12, slots=16, lm=lm, lm_weight=0.7, lm_bonus=0.2)
    flags = ["--beams", "4", "--ngram", str(arpa), "--lm-weight", "0.7", "--lm-bonus", "0.2"]
    lines = run(flags + ["--nbest", "3", "--scores"])
    bare = run(flags)
    assert len(lines) == len(bare) == 4
    for u, (l, b) in enumerate(zip(lines, bare)):
        n = len(want[u][0])
        assert set(b) == {"id", "token_ids"} and b["token_ids"] == l["token_ids"] and l["token_ids"][:n] == want[u][0].tolist()
        assert l["logprob"] == float(want.sequence_logprobs[u][0]) and l["lm_logprob"] == float(want.lm_logprobs[u][0])
        for h, r in enumerate(l["nbest"]):
            assert list(r) == ["ids", "score", "logprob", "avg_logprob", "lm_logprob"]
            assert r["ids"] == want[u][h].tolist() and r["score"] == float(want.sequence_scores[u][h]) and r["lm_logprob"] == float(want.lm_logprobs[u][h])
    with pytest.raises(SystemExit):
        tr.main(common + ["--ngram", str(arpa)])
    with pytest.raises(SystemExit):
        tr.main(common + ["--beams", "4", "--lm-weight", "0.5"])
    small = tmp_path / "small.arpa"
    P.NgramLM.train([[4, 5, 6]], 2, 30).to_arpa(small)
    with pytest.raises(SystemExit, match="--ngram .*81 ids"):  # a model over 30 ids: ids 30 .. 80 have no unigram
        tr.main(common + ["--beams", "4", "--ngram", str(small)])
    with pytest.raises(SystemExit, match="--ngram"):
        tr.main(common + ["--beams", "4", "--ngram", str(tmp_path / "missing.arpa")])
